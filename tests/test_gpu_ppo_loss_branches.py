"""The five copies of the clipped PPO2 loss and its hand-written backward pass, on an MI355X, every branch, coefficient and ragged batch against
float64 autograd of ppo2.ppo_loss (cases, inputs and reference: tests/ppo_loss_lib.py; tests/test_ppo_loss_reference.py checks those on the CPU).

  copy 1  irrl_ppo_loss_kernel<12>            through the C entry point (n_blocks free) and through ppo2._FusedPPOLoss
  copy 2  irrl_ppo_heads_loss_kernel<12, 48>  through ppo2._FusedHeadsLoss (N_BLOCKS patched) and once through the C entry point (mean_out / value_out)
  copy 3  irrl_mlp_ppo_kernel<KIND>           ppo2.mlp_ppo_grads, MLP_PRECISION "f32"
  copy 4  irrl_mlp_ppo_bf16_kernel<KIND, REC>     "bf16x3", IRRL_MLP_WAVES=4; REC through mlp_ppo_grads_flat(rec=)
  copy 5  irrl_mlp_ppo_bf16_pc_kernel<KIND, REC>  "bf16x3", wave pairs; REC likewise

Every sample sits in a chosen branch of the loss (P1 .. P7, V1 .. V5: ppo_loss_lib), mixed batches hold all of them, pure batches one; rows whose
branch is clipped out must come back EXACTLY zero, the clip fraction must count exactly the designed rows.  Batch sizes: 1, one below / at / one
above the tile (64 rows, 16 for the MLP kernels), and sizes that send a workgroup round its stride loop again (n_blocks 1 and 2); every per-sample
input lies in front of NaN rows, every per-row output in front of sentinel rows.

Bounds: per tensor max |kernel - f64| / max |f64| <= 2e-5 (copy 1, MLP f32) / 1e-4 (MLP bf16x3) / 2e-4 (heads kernel), the project's bounds for
these arithmetics; a tensor over its bound is held to 4 x the error of the float32 eager graph (of the float64 two-plane model for bf16x3) on the
same inputs, computed in the test.  Measured on an MI355X, worst tensor over all cases of a group:
  copy 1 (irrl_ppo_loss)        mixed: d_mean 2.7e-06, d_vpred 1.1e-07, d_logstd 2.1e-06;  pure: 3.5e-06, 1.1e-07, 3.6e-06
  copy 2 (irrl_ppo_heads_loss)  mixed: d_hpi 3.7e-06, d_hv 3.0e-07, d_wpi 2.1e-06, d_bpi 2.8e-06, d_wv 2.9e-07, d_bv 1.4e-06, d_logstd 3.6e-06;
                                pure: d_hpi 4.1e-06, d_hv 8.7e-06, d_wpi 2.4e-06, d_bpi 4.1e-06, d_wv 4.3e-06, d_bv 6.8e-07;  mean_out 3.0e-07, value_out 1.7e-07
  copy 3 (MLP f32)              mixed: 3.2e-06 (vf.b, n 15), every other tensor <= 2.0e-06;  pure: 9.1e-06 (vf_fc0.w)
  copies 4, 5 (MLP bf16x3; the four forms measure the same to every digit printed)
                                mixed: 2.2e-05 (pi.w, n 467) except vf.b at n 15 below;  pure: 2.0e-05 in the policy network, value network below
Two cases pass on the fallback bound (4 x the float64 model of the two-plane split), both in all four bf16x3 forms and in no other:
  * n = 15, rows 0 .. 14, coefficient set (0.1, 1.0, 0.0, 0.0, 2.5): vf.b -- ONE number, a sum of nine terms of both signs -- kernel 2.67e-04, model 2.27e-04
  * the pure P7 batch of the same set: R == ov, so v - R is dv, |dv| <= 0.04 against |v| ~ 1: vf_fc0.w 1.89e-04, vf_fc1.w 2.39e-04, vf.w 1.69e-04;
    model 2.35e-04, 2.50e-04, 2.30e-04
"""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppo_loss_lib as L

N_SETS = range(len(L.COEF_SETS))
HALF_LOG_2PI_E = 0.5 * (math.log(2.0 * math.pi) + 1.0)


def _dev():
    return torch.device("cuda")


def _worse(worst, errs):
    for k, e in errs.items():
        worst[k] = max(worst.get(k, 0.0), e)


def _hold(what, errs, bound, fallback):
    """every error within `bound`; one that is not, within 4 x the error of the fallback arithmetic on the same inputs (computed only then)"""
    over = {k: e for k, e in errs.items() if not e <= bound}
    if over:
        fb = fallback()
        print("\n[ppo loss %s] over %.0e: %s; fallback arithmetic: %s" % (what, bound, L.fmt(over), L.fmt({k: fb[k] for k in over})))
        for k, e in over.items():
            assert e <= 4.0 * fb[k], (what, k, e, bound, fb[k])


def _check_scalars(what, loss, stats, ref, loss_tol, rtol, atol):
    want = float(ref["loss"])
    got = float(loss.detach())
    assert abs(got - want) <= loss_tol * max(1.0, abs(want)), (what, got, want)
    np.testing.assert_allclose(stats.detach().double().cpu().numpy(), ref["stats"].numpy(), rtol=rtol, atol=atol, err_msg=str(what))


def _zero_rows(des, dev):
    return (torch.from_numpy(np.isin(des["pcls"], L.P_ZERO)).to(dev), torch.from_numpy(np.isin(des["vcls"], L.V_ZERO)).to(dev))


def _check_rows(what, g_pi, g_v, des):
    """row gradients of the policy / value term: exactly zero in the clipped-out rows, something in every other row, nothing but numbers"""
    pz, vz = _zero_rows(des, g_pi.device)
    g_v = g_v.reshape(len(vz), -1)
    assert torch.isfinite(g_pi).all() and torch.isfinite(g_v).all(), what
    assert not g_pi[pz].any(), (what, "policy rows", int(g_pi[pz].abs().amax(1).count_nonzero()))
    assert not g_v[vz].any(), (what, "value rows", int(g_v[vz].abs().amax(1).count_nonzero()))
    assert (g_pi[~pz].abs().amax(1) > 0).all() and (g_v[~vz].abs().amax(1) > 0).all(), what


# ---------------------------------------------------------------- copy 1 ----
def _loss_kernel(case, n_blocks):
    """irrl_ppo_loss straight through the C entry point -> d_mean, d_vpred (views in front of sentinel rows), partials [n_blocks + 1, 16]"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    from high_speed_quadrupedal_locomotion_by_irrl_amd._lib import ptr, stream_ptr
    dev, M, coef = _dev(), case["M"], case["coef"]
    t = {k: L.padded(case[k], dev) for k in L.LOSS_INPUTS}
    logstd, stats = case["logstd"].to(dev), L.adv_stats(coef).to(dev)
    d_mean = L.padded(torch.full((M, 12), L.SENTINEL), dev, fill=L.SENTINEL)
    d_v = L.padded(torch.full((M,), L.SENTINEL), dev, fill=L.SENTINEL)
    partials = torch.full((n_blocks + 1, 16), L.SENTINEL, device=dev)
    _lib.check(_lib.load().irrl_ppo_loss(M, 12, ptr(t["mean"]), ptr(logstd), ptr(t["vpred"]), ptr(t["actions"]), ptr(t["returns"]), ptr(t["old_values"]),
                                         ptr(t["old_neglogp"]), ptr(stats), coef.cliprange, coef.vf_coef, ptr(d_mean), ptr(d_v), ptr(partials), n_blocks,
                                         stream_ptr(dev)))
    torch.cuda.synchronize()
    return d_mean, d_v, partials


def _check_loss_kernel(case, n_blocks, worst):
    M, coef, ref, des = case["M"], case["coef"], case["ref"], case["design"]
    what = ("irrl_ppo_loss", M, tuple(coef), n_blocks, L.class_id(case.get("pure")))
    d_mean, d_v, partials = _loss_kernel(case, n_blocks)
    assert L.untouched_behind(d_mean) and L.untouched_behind(d_v) and bool((partials[n_blocks] == L.SENTINEL).all()), what
    sums = partials[:n_blocks].sum(0)
    logstd = case["logstd"].to(sums.device)
    pg, vf, kl, cf = sums[0] / M, sums[1] / M, sums[2] / M, sums[3] / M                    # as _FusedPPOLoss.forward forms them
    ent = (logstd + HALF_LOG_2PI_E).sum()
    loss = pg - ent * coef.ent_coef + vf * coef.vf_coef
    _check_scalars(what, loss, torch.stack([pg, vf, ent, kl, cf]), ref, L.LOSS_TOL, L.STATS_RTOL, L.STATS_ATOL)
    assert float(sums[3]) == L.clipfrac_count(des), (what, float(sums[3]), L.clipfrac_count(des))
    _check_rows(what, d_mean, d_v, des)
    d_logstd = (sums[4:] - coef.ent_coef).reshape(1, 12)
    errs = {"d_mean": L.rel_err(d_mean, ref["d_mean"]), "d_vpred": L.rel_err(d_v, ref["d_vpred"]), "d_logstd": L.rel_err(d_logstd, ref["d_logstd"])}
    _worse(worst, errs)

    def fallback():
        e32 = L.loss_eager_f32(case)
        return {k: L.rel_err(e32[k], ref[k]) for k in errs}
    _hold(what, errs, L.BOUNDS["loss_kernel"], fallback)


@pytest.mark.parametrize("M", L.LOSS_MS)
def test_loss_kernel_every_branch_coefficient_and_block_count_against_float64(M):
    """irrl_ppo_loss_kernel<12> at M x n_blocks in {1, 2, 2048} x every coefficient set, mixed batches: d_mean / d_vpred rows (exactly zero where
    the branch is clipped out), the partial sums -> loss, pg, vf, kl; clipfrac M == the designed count; d_logstd with the -ent_coef of
    _FusedPPOLoss.forward; sentinels behind M untouched.  M = 1000 on one workgroup: four trips of the stride loop, the last with a partial wave."""
    worst = {}
    for ci in N_SETS:
        case = L.make_loss_case(M, ci)
        for n_blocks in L.LOSS_BLOCKS:
            _check_loss_kernel(case, n_blocks, worst)
    print("\n[irrl_ppo_loss M %d] worst max |kernel - float64| / max |float64| over %d coefficient sets x n_blocks %s: %s"
          % (M, len(L.COEF_SETS), L.LOSS_BLOCKS, L.fmt(worst)))


def test_loss_kernel_pure_batches():
    """48 samples of ONE class: a wrong branch changes the whole tensor instead of hiding in a mix.  P3 / P4 / P7 alone: d_mean is zero everywhere
    and d_logstd == -ent_coef exactly; V2 / V4 alone: d_vpred is zero everywhere."""
    worst = {}
    for ci in N_SETS:
        coef = L.COEF_SETS[ci]
        for pure in L.PURE_CLASSES:
            if pure == ("P", 7) and float(L.adv_stats(coef)[0]) != 0.0:
                continue
            case = dict(L.make_loss_case(L.PURE_N, ci, pure), pure=pure)
            _check_loss_kernel(case, 1, worst)
            d_mean, d_v, partials = _loss_kernel(case, 2)
            if pure[0] == "P" and pure[1] in L.P_ZERO:
                assert not d_mean.any(), (ci, pure)
                assert torch.equal(partials[:2].sum(0)[4:] - coef.ent_coef, torch.full((12,), -coef.ent_coef, device=d_mean.device)), (ci, pure)
            if pure[0] == "V" and pure[1] in L.V_ZERO:
                assert not d_v.any(), (ci, pure)
    print("\n[irrl_ppo_loss pure batches of %d] worst over classes and coefficient sets: %s" % (L.PURE_N, L.fmt(worst)))


@pytest.mark.parametrize("ci", N_SETS)
def test_fused_ppo_loss_function_against_float64_with_a_scaled_upstream_gradient(ci):
    """ppo2._FusedPPOLoss.apply + autograd.grad at M = 257 (N_BLOCKS = 2048 as shipped): loss, statistics, and the three gradients under an
    upstream gradient of 1 and of 0.25"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import ppo2 as P2
    dev = _dev()
    case = L.make_loss_case(257, ci)
    coef, ref, des = case["coef"], case["ref"], case["design"]
    for scale in (1.0, 0.25):
        mean, vpred = (L.padded(case[k], dev).detach().requires_grad_() for k in ("mean", "vpred"))
        logstd = case["logstd"].to(dev).requires_grad_()
        rest = [L.padded(case[k], dev) for k in ("actions", "returns", "old_values", "old_neglogp")]
        loss, stats = P2._FusedPPOLoss.apply(mean, vpred, logstd, *rest, L.adv_stats(coef).to(dev), coef.cliprange, coef.ent_coef, coef.vf_coef)
        _check_scalars(("_FusedPPOLoss", ci), loss, stats, ref, L.LOSS_TOL, L.STATS_RTOL, L.STATS_ATOL)
        assert round(float(stats[4]) * 257) == L.clipfrac_count(des) and abs(float(stats[4]) * 257 - L.clipfrac_count(des)) < 1e-3
        g = dict(zip(("d_mean", "d_vpred", "d_logstd"), torch.autograd.grad(scale * loss, [mean, vpred, logstd])))
        _check_rows(("_FusedPPOLoss", ci, scale), g["d_mean"], g["d_vpred"], des)
        errs = {k: L.rel_err(g[k], scale * ref[k]) for k in g}
        print("\n[_FusedPPOLoss M 257, %s, upstream %.2f] %s" % (tuple(coef), scale, L.fmt(errs)))
        assert all(e <= L.BOUNDS["loss_kernel"] for e in errs.values()), errs


# ---------------------------------------------------------------- copy 2 ----
def _heads_function(case, n_blocks, monkeypatch, scale=1.0):
    """ppo2._FusedHeadsLoss with N_BLOCKS = n_blocks -> loss, stats, {name: gradient}"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import ppo2 as P2
    monkeypatch.setattr(P2._FusedHeadsLoss, "N_BLOCKS", n_blocks)
    dev, coef = _dev(), case["coef"]
    leaves = [L.padded(case[k], dev).detach().requires_grad_() for k in ("h_pi", "h_v")] + [case[k].to(dev).requires_grad_() for k in L.HEADS_WEIGHTS]
    rest = [L.padded(case[k], dev) for k in ("actions", "returns", "old_values", "old_neglogp")]
    loss, stats = P2._FusedHeadsLoss.apply(*leaves, *rest, L.adv_stats(coef).to(dev), coef.cliprange, coef.ent_coef, coef.vf_coef)
    grads = torch.autograd.grad(scale * loss, leaves)
    torch.cuda.synchronize()
    return loss, stats, dict(zip(L.HEADS_GRADS, grads))


def _check_heads(case, n_blocks, monkeypatch, worst, scale=1.0):
    M, coef, ref, des = case["M"], case["coef"], case["ref"], case["design"]
    what = ("_FusedHeadsLoss", M, tuple(coef), n_blocks, L.class_id(case.get("pure")), scale)
    loss, stats, g = _heads_function(case, n_blocks, monkeypatch, scale)
    _check_scalars(what, loss, stats, ref, L.LOSS_TOL, L.STATS_RTOL, L.STATS_ATOL)
    assert round(float(stats[4]) * M) == L.clipfrac_count(des) and abs(float(stats[4]) * M - L.clipfrac_count(des)) < 1e-3, what
    _check_rows(what, g["d_hpi"], g["d_hv"], des)
    errs = {k: L.rel_err(g[k], scale * ref[k]) for k in L.HEADS_GRADS}
    _worse(worst, errs)

    def fallback():
        e32 = L.heads_eager_f32(case)
        return {k: L.rel_err(e32[k], ref[k]) for k in errs}
    _hold(what, errs, L.BOUNDS["heads"], fallback)
    return g


@pytest.mark.parametrize("M", L.HEADS_MS)
def test_heads_kernel_every_branch_coefficient_and_block_count_against_float64(M, monkeypatch):
    """irrl_ppo_heads_loss_kernel<12, 48> through ppo2._FusedHeadsLoss at M x N_BLOCKS in {1, 2, 1024} x every coefficient set: d_hpi / d_hv rows
    (exactly zero where clipped out), d_wpi, d_bpi, d_wv, d_bv, d_logstd, loss, statistics, the clipfrac count.  M = 700 on one workgroup: 11 tiles
    over 4 waves, three trips, the ragged tile in the last trip with the fourth wave idle."""
    worst = {}
    for ci in N_SETS:
        case = L.make_heads_case(M, ci)
        for n_blocks in L.HEADS_BLOCKS:
            _check_heads(case, n_blocks, monkeypatch, worst)
    _check_heads(L.make_heads_case(M, 2), 2, monkeypatch, worst, scale=0.25)
    print("\n[irrl_ppo_heads_loss M %d] worst max |kernel - float64| / max |float64| over %d coefficient sets x N_BLOCKS %s: %s"
          % (M, len(L.COEF_SETS), L.HEADS_BLOCKS, L.fmt(worst)))


def test_heads_kernel_pure_batches(monkeypatch):
    """48 samples of one class; P3 / P4 / P7 alone: d_hpi, d_wpi, d_bpi are zero and d_logstd == -ent_coef exactly; V2 / V4 alone: d_hv, d_wv, d_bv"""
    worst = {}
    for ci in N_SETS:
        coef = L.COEF_SETS[ci]
        for pure in L.PURE_CLASSES:
            if pure == ("P", 7) and float(L.adv_stats(coef)[0]) != 0.0:
                continue
            g = _check_heads(dict(L.make_heads_case(L.PURE_N, ci, pure), pure=pure), 1, monkeypatch, worst)
            if pure[0] == "P" and pure[1] in L.P_ZERO:
                assert not g["d_hpi"].any() and not g["d_wpi"].any() and not g["d_bpi"].any(), (ci, pure)
                assert torch.equal(g["d_logstd"], torch.full_like(g["d_logstd"], -coef.ent_coef)), (ci, pure)
            if pure[0] == "V" and pure[1] in L.V_ZERO:
                assert not g["d_hv"].any() and not g["d_wv"].any() and not g["d_bv"].any(), (ci, pure)
    print("\n[irrl_ppo_heads_loss pure batches of %d] worst over classes and coefficient sets: %s" % (L.PURE_N, L.fmt(worst)))


@pytest.mark.parametrize("M,n_blocks", [(700, 1), (65, 2)])
def test_heads_kernel_writes_its_heads_when_asked(M, n_blocks):
    """The C entry point with mean_out / value_out (Python always passes NULL: the store path is otherwise never run): both against the float64
    heads, within the f32 level (a chain of 48 f32 FMAs: 2e-5 of the largest entry), rows behind M untouched in all four per-row outputs; the
    row gradients as through the Function."""
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    from high_speed_quadrupedal_locomotion_by_irrl_amd._lib import ptr, stream_ptr
    dev = _dev()
    case = L.make_heads_case(M, 0)
    coef, ref, des = case["coef"], case["ref"], case["design"]
    t = {k: L.padded(case[k], dev) for k in L.HEADS_INPUTS}
    w = {k: case[k].to(dev).contiguous() for k in L.HEADS_WEIGHTS}
    out = {"d_hpi": (M, 48), "d_hv": (M, 48), "mean": (M, 12), "value": (M,)}
    out = {k: L.padded(torch.full(s, L.SENTINEL), dev, fill=L.SENTINEL) for k, s in out.items()}
    P = 4 + 12 + 12 + 1 + 48 + 48 * 12
    partials = torch.full((n_blocks + 1, P), L.SENTINEL, device=dev)
    _lib.check(_lib.load().irrl_ppo_heads_loss(M, 12, 48, ptr(t["h_pi"]), ptr(t["h_v"]), ptr(w["pi_w"]), ptr(w["pi_b"]), ptr(w["vf_w"]), ptr(w["vf_b"]),
                                               ptr(w["logstd"]), ptr(t["actions"]), ptr(t["returns"]), ptr(t["old_values"]), ptr(t["old_neglogp"]),
                                               ptr(L.adv_stats(coef).to(dev)), coef.cliprange, coef.vf_coef, ptr(out["d_hpi"]), ptr(out["d_hv"]),
                                               ptr(out["mean"]), ptr(out["value"]), ptr(partials), n_blocks, stream_ptr(dev)))
    torch.cuda.synchronize()
    for k, o in out.items():
        assert L.untouched_behind(o), k
    assert bool((partials[n_blocks] == L.SENTINEL).all()) and torch.isfinite(partials[:n_blocks]).all()
    _check_rows(("irrl_ppo_heads_loss", M), out["d_hpi"], out["d_hv"], des)
    assert float(partials[:n_blocks].sum(0)[3]) == L.clipfrac_count(des)
    errs = {"mean_out": L.rel_err(out["mean"], ref["mean"]), "value_out": L.rel_err(out["value"], ref["value"]),
            "d_hpi": L.rel_err(out["d_hpi"], ref["d_hpi"]), "d_hv": L.rel_err(out["d_hv"], ref["d_hv"])}
    print("\n[irrl_ppo_heads_loss with mean_out / value_out, M %d, n_blocks %d] %s" % (M, n_blocks, L.fmt(errs)))
    assert errs["mean_out"] <= 2e-5 and errs["value_out"] <= 2e-5 and errs["d_hpi"] <= L.BOUNDS["heads"] and errs["d_hv"] <= L.BOUNDS["heads"], errs


# ---------------------------------------------------------------- copies 3 - 5 ----
class _MlpRun(object):
    """One MlpPolicy gradient-kernel form on the device: the policy, and for the packed-record forms its flat buffers"""

    def __init__(self, form, policy, monkeypatch):
        from high_speed_quadrupedal_locomotion_by_irrl_amd import ppo2 as P2
        self.P2, self.form = P2, form
        monkeypatch.setattr(P2, "MLP_PRECISION", form.prec)
        monkeypatch.setenv("IRRL_MLP_WAVES", form.waves)
        self.pol = copy.deepcopy(policy).to(_dev())
        self.flat = P2.FlatParams(self.pol) if form.rec else None

    def __call__(self, case, n_blocks):
        """-> loss, stats [pg, vf, entropy, approxkl, clipfrac], {name: gradient}, the clip count if the form hands out the raw sum"""
        P2, dev, n, coef = self.P2, _dev(), case["n"], case["coef"]
        full = [case[k].to(dev) for k in L.MLP_INPUTS]
        index = case["index"].to(dev) if case["index"] is not None else None
        arrays = full if index is not None else [t[:n] for t in full]          # not indexed: the leading rows of a longer allocation
        stats = L.adv_stats(coef).to(dev)
        assert P2.mlp_ppo_grads_supported(self.pol, arrays[0])
        names = dict(zip((id(p) for p in L.mlp_params(self.pol)), L.MLP_PARAM_NAMES))
        if not self.form.rec:
            loss, st, grads = P2.mlp_ppo_grads(self.pol, *arrays, stats, coef.cliprange, coef.ent_coef, coef.vf_coef, index=index, n_blocks=n_blocks)
            torch.cuda.synchronize()
            assert len(grads) == 13
            return loss, st, {names[id(p)]: g for p, g in grads.items()}, None
        rec = P2.mlp_pack_records(*full)
        self.flat.grad.fill_(float("nan"))            # every slot of the 13 gradients and of the statistics is written, not added to
        row = P2.mlp_ppo_grads_flat(self.pol, self.flat, *arrays, stats, coef.cliprange, coef.ent_coef, coef.vf_coef, index, n_blocks=n_blocks, rec=rec)
        torch.cuda.synchronize()
        st = P2.mlp_stats_rows([row], n, 12)[0]
        loss = st[0] - st[2] * coef.ent_coef + st[1] * coef.vf_coef
        grads = {names[id(p)]: gv.clone() for p, gv in zip(self.flat.params, self.flat.grad_views) if id(p) in names}
        return loss, st, grads, float(row[2])


def _check_mlp(run, case, n_blocks, worst, indexed):
    form, n, coef, ref, des = run.form, case["n"], case["coef"], case["ref"], case["design"]
    what = (form.name, n, "indexed" if indexed else "rows", tuple(coef), n_blocks, L.class_id(case.get("pure")))
    tol = L.BOUNDS[form.prec]
    loss, st, grads, clip_sum = run(case, n_blocks)
    _check_scalars(what, loss, st, ref, tol, 10 * tol, tol)
    count = L.clipfrac_count(des)
    assert round(float(st[4]) * n) == count and abs(float(st[4]) * n - count) < 1e-3, (what, float(st[4]) * n, count)
    assert clip_sum is None or clip_sum == count, (what, clip_sum, count)
    assert set(grads) == set(L.MLP_PARAM_NAMES)
    errs = {}
    for k in L.MLP_PARAM_NAMES:
        assert grads[k].shape == ref["grads"][k].shape and torch.isfinite(grads[k]).all(), (what, k)
        errs[k] = L.rel_err(grads[k], ref["grads"][k])
    _worse(worst, errs)

    def fallback():
        other = L.mlp_eager_f32(case)[2] if form.prec == "f32" else L.mlp_bf16x3_model(case)[2]
        return {k: L.rel_err(other[k], ref["grads"][k]) for k in errs}
    _hold(what, errs, tol, fallback)
    return st, grads


@pytest.mark.parametrize("n", L.MLP_NS)
@pytest.mark.parametrize("form", L.MLP_FORMS, ids=lambda f: f.name)
def test_mlp_gradient_kernels_every_branch_coefficient_and_block_count_against_float64(form, n, monkeypatch):
    """irrl_mlp_ppo_kernel / irrl_mlp_ppo_bf16_kernel<., REC> / irrl_mlp_ppo_bf16_pc_kernel<., REC> at n x n_blocks in {1, 2, 256} x indexed or not x
    every coefficient set: all 13 gradients, the loss and the statistics against float64 -- each form on its own, not form against form.  n = 1
    and 15 .. 17 leave most lanes of the only tiles without a sample (their loads are clamped to the last row: a missing `valid` guard counts that
    row again); 197 and 467 on one workgroup send its waves round the tile loop 4 and 8 times, the last tile ragged."""
    run = _MlpRun(form, L.make_mlp_policy(L.seed_of("mlp-policy", n)), monkeypatch)
    worst = {}
    for indexed in (False, True):
        for ci in N_SETS:
            case = L.make_mlp_case(n, indexed, ci)
            for n_blocks in L.MLP_BLOCKS:
                _check_mlp(run, case, n_blocks, worst, indexed)
    print("\n[mlp gradients %s, n %d] worst max |kernel - float64| / max |float64| over indexed or not x %d coefficient sets x n_blocks %s:\n    %s"
          % (form.name, n, len(L.COEF_SETS), L.MLP_BLOCKS, L.fmt(worst)))


@pytest.mark.parametrize("form", L.MLP_FORMS, ids=lambda f: f.name)
def test_mlp_gradient_kernels_pure_batches(form, monkeypatch):
    """48 samples of ONE class, every class, every coefficient set, each against float64.  P3 / P4 / P7 alone: every policy-network gradient is
    exactly zero, d logstd == -ent_coef exactly, clipfrac == 1; V2 / V4 alone: every value-network gradient is exactly zero."""
    run = _MlpRun(form, L.make_mlp_policy(L.seed_of("mlp-policy", L.PURE_N)), monkeypatch)
    worst = {}
    for ci in N_SETS:
        coef = L.COEF_SETS[ci]
        for pure in L.PURE_CLASSES:
            if pure == ("P", 7) and float(L.adv_stats(coef)[0]) != 0.0:
                continue
            case = dict(L.make_mlp_case(L.PURE_N, False, ci, pure), pure=pure)
            st, g = _check_mlp(run, case, 2, worst, False)
            if pure[0] == "P" and pure[1] in L.P_ZERO:
                for k in L.MLP_POLICY_NET:
                    assert not g[k].any(), (form.name, ci, pure, k, float(g[k].abs().max()))
                assert torch.equal(g["logstd"], torch.full_like(g["logstd"], -coef.ent_coef)), (form.name, ci, pure, g["logstd"])
                assert float(st[4]) == 1.0
            if pure[0] == "V" and pure[1] in L.V_ZERO:
                for k in L.MLP_VALUE_NET:
                    assert not g[k].any(), (form.name, ci, pure, k, float(g[k].abs().max()))
    print("\n[mlp gradients %s, pure batches of %d] worst over classes and coefficient sets:\n    %s" % (form.name, L.PURE_N, L.fmt(worst)))
