"""CPU side of tests/test_gpu_ppo_loss_branches.py: the engineered batches and the float64 reference that module relies on (tests/ppo_loss_lib.py),
checked without a GPU.

  * the float64 autograd reference equals a straight numpy transcription of ppo2.ppo_loss -- loss, statistics, and the row gradients the branch
    table predicts (zero in the clipped-out classes, adv ratio / M and vf_coef (v - R) / M in the active ones);
  * every sample of every case lands in its DESIGNED class, computed from the float64 forward values and again from the float32 eager ones, with
    the margins of ppo_loss_lib's docstring; every class occurs in the mixed batches; every pure batch is pure;
  * autograd's gradient is exactly 0 in the P3 / P4 / P7 / V2 / V4 rows, which is what entitles the GPU module to assert exact zeros;
  * every case is conditioned well enough for its bound to mean something: the float32 eager graph stays under HALF of the bound the f32 kernels
    are held to, per tensor (most of what it shows is exp(old_neglogp - neglogp) at neglogp ~ 20: 1 .. 4e-6); the float64 model of the bf16x3
    arithmetic under half of 1e-4 on the mixed batches from 197 samples on.  Where the model itself passes 1e-4 -- the value network under a pure
    P7 batch, whose v - R is dv by construction, |dv| < c, against |v| ~ 1; the one-number bias gradient of the value head at n = 15 -- the GPU
    module's bound for the bf16x3 forms is four times the model's error, as the issue's fallback rule has it.
"""
import numpy as np
import pytest
import torch

import ppo_loss_lib as L

N_SETS = range(len(L.COEF_SETS))


def _check_design(case, forward, what):
    """classes from float64 and float32 forward values == the design; margins; counts"""
    des, coef = case["design"], case["coef"]
    M = len(des["pcls"])
    for dtype in (torch.float64, torch.float32):
        nlp, v = forward(case, dtype)
        rows = case.get("rows")
        sel = (lambda t: t[rows]) if rows is not None else (lambda t: t)
        got = L.classify(nlp, v, sel(case["returns"]).to(dtype), sel(case["old_values"]).to(dtype), sel(case["old_neglogp"]).to(dtype), coef)
        assert np.array_equal(got["pcls"], des["pcls"]), (what, dtype, np.nonzero(got["pcls"] != des["pcls"])[0][:5])
        assert np.array_equal(got["vcls"], des["vcls"]), (what, dtype, np.nonzero(got["vcls"] != des["vcls"])[0][:5])
        assert got["ratio_margin"].min() >= L.MARGIN, (what, dtype, got["ratio_margin"].min())
        assert got["dv_margin"].min() >= L.MARGIN, (what, dtype, got["dv_margin"].min())
        p7 = des["pcls"] == 7
        assert (got["adv"][p7] == 0.0).all()                     # exactly, in both precisions
        assert (np.abs(got["adv"][~p7]) >= L.ADV_MARGIN).all(), (what, dtype, np.abs(got["adv"][~p7]).min())
        clipped_v = des["vcls"] != 1
        assert (got["l_margin"][clipped_v] >= L.MARGIN).all(), (what, dtype, got["l_margin"][clipped_v].min())
        assert int((np.abs(got["ratio"] - 1.0) > coef.cliprange).sum()) == L.clipfrac_count(des)
    return M


def _check_counts(des, coef, pure, M):
    """mixed: every class of the table occurs (P7 where a_mean == 0), at least 8 times once the batch has 8 samples per feasible pair, at least once
    when it has one per pair; pure: one class only"""
    pairs = L.feasible_pairs(coef)
    p_want = [p for p in L.P_CLASSES if p != 7 or float(L.adv_stats(coef)[0]) == 0.0]
    assert {p for p, _ in pairs} == set(p_want) and {v for _, v in pairs} == set(L.V_CLASSES)
    if pure is None:
        least = 8 if M >= 8 * len(pairs) else 1 if M >= len(pairs) else 0
        for p in p_want:
            assert int((des["pcls"] == p).sum()) >= least, (coef, M, "P", p)
        for v in L.V_CLASSES:
            assert int((des["vcls"] == v).sum()) >= least, (coef, M, "V", v)
        assert (des["pcls"][0], des["vcls"][0]) == (1, 5)        # a batch of one sample is active in both terms
    else:
        assert (des["pcls" if pure[0] == "P" else "vcls"] == pure[1]).all()


def _pure_list(coef):
    return [pc for pc in L.PURE_CLASSES if pc != ("P", 7) or float(L.adv_stats(coef)[0]) == 0.0]


def test_coefficient_sets_and_pairs():
    assert L.COEF_SETS[:3] == [L.Coef(0.2, 0.5, 0.01, 0.0, 1.0), L.Coef(0.1, 1.0, 0.0, 0.3, 2.5), L.Coef(0.3, 0.25, 0.05, -0.4, 0.6)]
    assert sum(float(L.adv_stats(c)[0]) == 0.0 for c in L.COEF_SETS) >= 2          # P7 at two clip ranges
    for coef in L.COEF_SETS:
        pairs = L.feasible_pairs(coef)
        print("\n[ppo loss pairs %s] %d pairs: %s" % (tuple(coef), len(pairs), " ".join("P%dV%d" % k for k in pairs)))
        assert max(L.LOSS_MS) >= 8 * len(pairs) and max(L.HEADS_MS) >= 8 * len(pairs) and L.MLP_NS[-2] >= 8 * len(pairs)
        assert all(L.S_LO <= lo <= hi <= L.S_HI for lo, hi in pairs.values())


@pytest.mark.parametrize("ci", N_SETS)
@pytest.mark.parametrize("M", L.LOSS_MS)
def test_loss_kernel_cases_are_what_they_are_designed_to_be(M, ci):
    case = L.make_loss_case(M, ci)
    _check_design(case, L.loss_forward, ("loss", M, ci))
    _check_counts(case["design"], case["coef"], None, M)


@pytest.mark.parametrize("ci", N_SETS)
@pytest.mark.parametrize("M", L.HEADS_MS)
def test_heads_kernel_cases_are_what_they_are_designed_to_be(M, ci):
    case = L.make_heads_case(M, ci)
    _check_design(case, L.heads_forward, ("heads", M, ci))
    _check_counts(case["design"], case["coef"], None, M)
    assert float(case["h_pi"].abs().max()) < 1.0 and float(case["h_v"].abs().max()) < 1.0


@pytest.mark.parametrize("ci", N_SETS)
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("n", L.MLP_NS)
def test_mlp_kernel_cases_are_what_they_are_designed_to_be(n, indexed, ci):
    case = L.make_mlp_case(n, indexed, ci)
    _check_design(case, L.mlp_forward, ("mlp", n, indexed, ci))
    _check_counts(case["design"], case["coef"], None, n)
    # every row outside the minibatch holds NaN in all five arrays; the minibatch's rows hold none
    total = case["returns"].shape[0]
    assert total == (2 * n + 77 if indexed else n + L.PAD_ROWS)
    used = torch.zeros(total, dtype=torch.bool)
    used[case["rows"]] = True
    assert int(used.sum()) == n
    for name in L.MLP_INPUTS:
        bad = torch.isnan(case[name]).reshape(total, -1)
        assert bad[~used].all() and not bad[used].any(), name
    if indexed:
        assert not torch.equal(case["index"], torch.sort(case["index"])[0]) or n == 1


@pytest.mark.parametrize("ci", N_SETS)
def test_pure_batches_are_pure(ci):
    coef = L.COEF_SETS[ci]
    for pure in _pure_list(coef):
        for make, fwd, what in ((L.make_loss_case, L.loss_forward, "loss"), (L.make_heads_case, L.heads_forward, "heads")):
            case = make(L.PURE_N, ci, pure)
            _check_design(case, fwd, (what, ci, pure))
            _check_counts(case["design"], coef, pure, L.PURE_N)
        case = L.make_mlp_case(L.PURE_N, False, ci, pure)
        _check_design(case, L.mlp_forward, ("mlp", ci, pure))
        _check_counts(case["design"], coef, pure, L.PURE_N)
        if pure in (("P", 3), ("P", 4)):
            assert L.clipfrac_count(case["design"]) == L.PURE_N
    if float(L.adv_stats(coef)[0]) != 0.0:
        with pytest.raises(AssertionError):
            L.design(L.PURE_N, coef, 1, ("P", 7))               # not constructible: said so, not silently something else


def _np(t):
    return t.detach().double().numpy()


@pytest.mark.parametrize("ci", N_SETS)
@pytest.mark.parametrize("M", [1, 65, 1000])
def test_float64_reference_equals_a_numpy_transcription_and_the_branch_table(M, ci):
    """copy 1's reference: loss and statistics to 1e-13; d loss / d mean and d loss / d vpred rows equal the branch table's row gradients pushed
    through d neglogp / d mean = -(a - mean) / std^2 -- zero rows included"""
    case = L.make_loss_case(M, ci)
    ref, des, coef = case["ref"], case["design"], case["coef"]
    a = {k: _np(case[k]) for k in ("mean", "vpred", "logstd", "actions", "returns", "old_values", "old_neglogp")}
    loss, stats, d_nlp, d_v = L.numpy_loss(a["mean"], a["vpred"], a["logstd"], a["actions"], a["returns"], a["old_values"], a["old_neglogp"], coef,
                                           des["pcls"], des["vcls"])
    assert abs(float(ref["loss"]) - loss) <= 1e-13 * max(1.0, abs(loss))
    assert np.abs(_np(ref["stats"]) - stats).max() <= 1e-13 * max(1.0, np.abs(stats).max())
    assert stats[4] * M == pytest.approx(L.clipfrac_count(des), abs=1e-9)
    d_mean = d_nlp[:, None] * (-(a["actions"] - a["mean"]) / np.exp(2.0 * a["logstd"]))
    scale = max(np.abs(d_mean).max(), 1e-300)
    assert np.abs(_np(ref["d_mean"]) - d_mean).max() <= 1e-12 * scale
    assert np.abs(_np(ref["d_vpred"]) - d_v).max() <= 1e-12 * max(np.abs(d_v).max(), 1e-300)
    z = ((a["actions"] - a["mean"]) / np.exp(a["logstd"])) ** 2
    d_ls = (d_nlp[:, None] * (1.0 - z)).sum(0) - coef.ent_coef
    assert np.abs(_np(ref["d_logstd"]).reshape(-1) - d_ls.reshape(-1)).max() <= 1e-12 * max(1.0, np.abs(d_ls).max())


def _zero_rows(des):
    return np.isin(des["pcls"], L.P_ZERO), np.isin(des["vcls"], L.V_ZERO)


@pytest.mark.parametrize("ci", N_SETS)
def test_autograd_gradient_is_exactly_zero_in_the_clipped_out_rows(ci):
    """P3 / P4 / P7 rows of d_mean (d_hpi), V2 / V4 rows of d_vpred (d_hv): == 0.0 in the float64 reference, and nonzero in every other row"""
    for case, pi_rows, v_rows in ((L.make_loss_case(1000, ci), "d_mean", "d_vpred"), (L.make_heads_case(700, ci), "d_hpi", "d_hv")):
        pz, vz = _zero_rows(case["design"])
        gp, gv = _np(case["ref"][pi_rows]), _np(case["ref"][v_rows]).reshape(len(vz), -1)
        assert pz.any() and vz.any() and (~pz).any() and (~vz).any()
        assert (gp[pz] == 0.0).all() and (gv[vz] == 0.0).all()
        assert (np.abs(gp[~pz]).max(1) > 0.0).all() and (np.abs(gv[~vz]).max(1) > 0.0).all()


@pytest.mark.parametrize("ci", N_SETS)
def test_pure_clipped_out_batches_have_exactly_zero_network_gradients_in_the_reference(ci):
    """MlpPolicy: a batch of P3 / P4 / P7 alone leaves the policy network without any gradient (d logstd = -ent_coef from the entropy alone), a
    batch of V2 / V4 alone the value network; every other pure batch moves its network"""
    coef = L.COEF_SETS[ci]
    for pure in _pure_list(coef):
        g = L.make_mlp_case(L.PURE_N, False, ci, pure)["ref"]["grads"]
        pi_max = max(float(g[k].abs().max()) for k in L.MLP_POLICY_NET)
        v_max = max(float(g[k].abs().max()) for k in L.MLP_VALUE_NET)
        if pure[0] == "P":
            assert (pi_max == 0.0) == (pure[1] in L.P_ZERO), (pure, pi_max)
            if pure[1] in L.P_ZERO:
                assert float((g["logstd"] + coef.ent_coef).abs().max()) <= 1e-15
        else:
            assert (v_max == 0.0) == (pure[1] in L.V_ZERO), (pure, v_max)


def _every_case(ci):
    """(kind, key, case) of every case the GPU module runs under coefficient set ci"""
    for pure in [None] + _pure_list(L.COEF_SETS[ci]):
        for M in (L.LOSS_MS if pure is None else (L.PURE_N,)):
            yield "loss", (M, ci, pure), L.make_loss_case(M, ci, pure)
        for M in (L.HEADS_MS if pure is None else (L.PURE_N,)):
            yield "heads", (M, ci, pure), L.make_heads_case(M, ci, pure)
        for n in (L.MLP_NS if pure is None else (L.PURE_N,)):
            for indexed in ((False, True) if pure is None else (False,)):
                yield "mlp", (n, indexed, ci, pure), L.make_mlp_case(n, indexed, ci, pure)


@pytest.mark.parametrize("ci", N_SETS)
def test_eager_f32_stays_under_half_of_the_f32_kernel_bounds(ci):
    worst = {}
    for kind, key, case in _every_case(ci):
        if kind == "mlp":
            out, ref, bound = L.mlp_eager_f32(case)[2], case["ref"]["grads"], L.BOUNDS["f32"]
        else:
            out, ref = (L.loss_eager_f32 if kind == "loss" else L.heads_eager_f32)(case), case["ref"]
            bound = L.BOUNDS["loss_kernel" if kind == "loss" else "heads"]
        for k, g in out.items():
            e = L.rel_err(g, ref[k])
            assert e <= 0.5 * bound, (kind, key, k, e, bound)
            worst[kind] = max(worst.get(kind, 0.0), e)
    print("\n[ppo loss eager f32 on the CPU, %s] worst max |f32 - float64| / max |float64| over all cases: %s" % (tuple(L.COEF_SETS[ci]), L.fmt(worst)))


@pytest.mark.parametrize("ci", N_SETS)
def test_bf16x3_model_stays_under_half_of_the_bf16x3_bound_on_the_larger_mixed_batches(ci):
    worst, over = 0.0, []
    for kind, key, case in _every_case(ci):
        if kind != "mlp":
            continue
        model = L.mlp_bf16x3_model(case)[2]
        errs = {k: L.rel_err(model[k], case["ref"]["grads"][k]) for k in L.MLP_PARAM_NAMES}
        over += [(key, k, "%.2e" % e) for k, e in errs.items() if e > L.BOUNDS["bf16x3"]]
        if key[3] is None and key[0] >= 197:
            worst = max(worst, max(errs.values()))
            assert max(errs.values()) <= 0.5 * L.BOUNDS["bf16x3"], (key, errs)
    print("\n[ppo loss bf16x3 float64 model, %s] worst on mixed n >= 197: %.2e; model itself over 1e-4 (fallback bound on the GPU): %s"
          % (tuple(L.COEF_SETS[ci]), worst, over))


def test_padding_helpers():
    t = torch.arange(6.0).reshape(3, 2)
    p = L.padded(t)
    assert torch.equal(p, t) and p._base.shape == (3 + L.PAD_ROWS, 2) and torch.isnan(p._base[3:]).all() and p.is_contiguous()
    o = L.padded(torch.zeros(3), fill=L.SENTINEL)
    assert L.untouched_behind(o)
    o._base[3] = 0.0
    assert not L.untouched_behind(o)


def test_bf16x3_model_and_eager_f32_are_what_the_fallback_bounds_assume():
    """the two-plane model sits between the f32 level and a one-plane bf16 arithmetic; the float32 eager graph at the f32 level"""
    case = L.make_mlp_case(197, True, 0)
    ref = case["ref"]["grads"]
    model = L.mlp_bf16x3_model(case)[2]
    eager = L.mlp_eager_f32(case)[2]
    em = {k: L.rel_err(model[k], ref[k]) for k in L.MLP_PARAM_NAMES}
    ee = {k: L.rel_err(eager[k], ref[k]) for k in L.MLP_PARAM_NAMES}
    print("\n[mlp bf16x3 float64 model, n 197] %s\n[mlp eager f32, n 197] %s" % (L.fmt(em), L.fmt(ee)))
    assert all(e < 2.0 ** -12 for e in em.values()) and max(em.values()) > 1e-8
    assert all(e < 1e-4 for e in ee.values())
