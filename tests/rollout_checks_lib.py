"""Shared pieces of tests/test_gpu_rollout_replay.py, tests/test_gpu_rollout_ragged.py (MI355X) and tests/test_rollout_ragged_reference.py (CPU):
the checks a recorded rollout is put through against its float64 replay (tests/rollout_replay_lib.py), written once, and the ragged pools.

  check_replay        the six checks of test_device_rollout_is_what_a_float64_replay_of_its_observations_gives on the rollouts of one case
  zero_lr_update      update(batch, 0.0, cliprange) on a recorded batch: parameters untouched, clipfrac 0, statistics as expected_stats
  RAGGED_PLANS        pool sizes whose last wave owns one, two or three robots (a wave owns four, a workgroup sixteen) with the designed episode
                      ends of each: every plan ends an episode inside the partial wave
"""
import numpy as np
import torch

import lstm_forms_lib as FL
import rollout_replay_lib as R

CLIPRANGE = 0.2
SAMPLER_TOL = 2e-3          # test_fused_policy_step_kernel_noise_is_the_counter_rng

# N -> {robot: row} in the sense of rollout_replay_lib.PLAN.  1: one robot, no full wave; 6: the partial wave holds robots 4, 5; 7: robots 4, 5, 6;
# 37: robot 36 alone in its wave, behind two full workgroups and one full wave (32 .. 35), in which an episode ends too
RAGGED_PLANS = {1: {0: 5}, 6: {1: 1, 4: 11, 5: 24}, 7: {0: 24, 4: 2, 6: 23}, 37: {0: 1, 17: 5, 33: 11, 36: 17, 35: 23, 20: 24}}
# the full pool (a multiple of 16 robots) whose first N robots the ragged pool must be
FULL_POOL = {1: 16, 6: 16, 7: 16, 37: 48}
LOGSTD_RANGE = (-1.0, 0.5)
ROLLOUT_KEYS = ("obs", "actions", "values", "true_reward", "masks", "neglogpacs", "returns", "states")


def plan_is_about_the_partial_wave(n, plan):
    """the plan ends an episode on a robot of the last, partial wave (and, where there is one, on a robot of a full wave)"""
    first = (n // 4) * 4
    assert n % 4 and max(plan) < n and any(i >= first for i in plan)
    assert first == 0 or any(i < first for i in plan)
    return True


def assert_actor_only_equals(got, want, tag):
    """the comparisons of test_graph_capture_warmup_leaves_no_trace_and_setters_invalidate_the_graph for the actor-only rollout: the actor side
    bit for bit; values, returns and the critic's half of the carried state at that test's 2e-5 of their scale (the sequence kernels' error)"""
    for k in ("obs", "actions", "true_reward", "masks", "neglogpacs"):
        assert torch.equal(got[k], want[k]), (tag, k)
    sa, se = got["states"], want["states"]
    assert torch.equal(sa[:, :192], se[:, :192]), tag
    assert float((sa[:, 192:] - se[:, 192:]).abs().max()) < 2e-5 * (1.0 + float(se[:, 192:].abs().max())), tag
    for k in ("values", "returns"):
        a, b = got[k], want[k]
        assert float((a - b).abs().max()) < 2e-5 * (1.0 + float(b.abs().max())), (tag, k, float((a - b).abs().max()))


def hold(what, errs, bounds, fallback):
    """every error within its bound; one that is not, within 4 x the error of the float32 eager replay on the same batch (computed only then)"""
    over = {k: e for k, e in errs.items() if not e <= bounds[k]}
    if over:
        fb = fallback()
        print("\n[rollout replay %s] over its bound: %s; float32 eager replay: %s" % (what, FL.fmt(over), FL.fmt({k: fb[k] for k in over})))
        for k, e in over.items():
            assert e <= 4.0 * fb[k], (what, k, e, bounds[k], fb[k])


def f32_replay_errors(pol, batch, last, rep):
    """the errors of `replay_errors` / `returns_errors` for the float32 eager replay in place of the recorded numbers"""
    r32 = R.replay(pol, batch, last, dtype=torch.float32)
    fake_batch = dict(batch, values=r32["value"], neglogpacs=r32["neglogp"])
    fake_last = dict(last, result=r32["last_value"], states=r32["state"])
    return R.replay_errors(pol, fake_batch, fake_last, rep)


def check_replay(model, rollouts, plan, tag, logstd_range):
    """The recorded rollouts [(batch, last, rng_base)] of consecutive run() calls under `plan` against their float64 replay:
    1. exactly the designed episode ends, the carried done flags and state; 2. the sampler of every row, env and slot; 3. + 4. recorded neglogp /
    values, the carried state by halves and the bootstrap value; 5. returns and advantages; 6. the same replay with `masks` one row early misses
    on every ended robot.  -> the worst measured value of each over the rollouts ("power_value", "power_returns": the least)"""
    pol, T = model.policy, R.T_STEPS
    N = rollouts[0][0]["masks"].shape[1]
    worst = {}

    def note(key, v, least=False):
        worst[key] = v if key not in worst else (min if least else max)(worst[key], v)
    for r, (batch, last, rng_base) in enumerate(rollouts):
        what = tuple(tag) + (r,)
        # 1. conditions: exactly the designed episode ends
        ends = R.realised_ends(batch, last)
        assert ends == {i: [k] for i, k in plan.items()}, (what, ends)
        want_last = torch.tensor([plan.get(i) == T for i in range(N)], device=last["dones"].device)
        assert torch.equal(last["dones"].bool(), want_last) and bool(want_last.any()) == (T in plan.values())
        if r:
            assert torch.equal(batch["masks"][0], rollouts[r - 1][1]["dones"].to(batch["masks"].dtype))
            assert bool(batch["masks"][0].any()) == (T in plan.values())
        else:
            assert not batch["masks"][0].any()
        if pol.recurrent:
            assert torch.equal(batch["states"], rollouts[r - 1][1]["states"]) if r else not batch["states"].any()
        rep = R.replay(pol, batch, last)
        if logstd_range is not None:
            assert float(rep["logstd"].min()) == logstd_range[0] and float(rep["logstd"].max()) == logstd_range[1]
        # 2. the sampler: every row, env and slot
        s_err = R.sampler_error(model, batch, rep, rng_base)
        # 3. + 4. old neglogp / values, carried state by halves, bootstrap
        errs = R.replay_errors(pol, batch, last, rep)
        # 5. returns
        g_errs = R.returns_errors(batch, last, rep)
        # 6. power
        power = R.power_errors(pol, batch, last, rep)
        print("\n[rollout replay %s rollout %d] sampler %.2e  %s  %s  masks one row early: values (least / largest over the ended robots) %s, returns (least) %.1e"
              % ("-".join(str(v) for v in tag), r, s_err, FL.fmt(errs), FL.fmt(g_errs),
                 "%.1e / %.1e" % (min(p[0] for p in power.values()), max(p[0] for p in power.values())) if pol.recurrent else "n/a",
                 min(p[1] for p in power.values())))
        assert s_err <= SAMPLER_TOL, (what, s_err)
        assert pol.recurrent == ("state_v" in errs)
        hold(what, errs, R.REPLAY_TOL, lambda: f32_replay_errors(pol, batch, last, rep))
        assert g_errs["returns"] <= R.RETURNS_TOL and g_errs["advantages"] <= R.RETURNS_TOL, (what, g_errs)
        assert set(power) == set(plan)
        for i, (_, r_err) in power.items():
            assert r_err >= R.POWER * R.RETURNS_TOL, (what, i, r_err)
        # (the values' error is, as in 3., the largest over the tensor -- here the ended robots' columns: how far ONE robot's value moves when its
        # state is cleared a row early is the policy's business, 1.3e-03 .. 3.3e-02 in the cases of the 40-robot pool)
        assert not pol.recurrent or max(p[0] for p in power.values()) >= R.POWER * R.REPLAY_TOL["value"], (what, power)
        note("sampler", s_err)
        for k, e in list(errs.items()) + list(g_errs.items()):
            note(k, e)
        note("power_returns", min(p[1] for p in power.values()), least=True)
        if pol.recurrent:
            note("power_value", max(p[0] for p in power.values()), least=True)
    return worst


def zero_lr_update(model, batch, last, rep, tol, d_new=None):
    """update(batch, 0.0, cliprange) on the recorded batch -> printed line; asserts: every parameter bit-identical afterwards, clipfrac exactly 0,
    pg / vf / entropy as rollout_replay_lib.expected_stats within (10 tol, tol), approxkl <= (d_old + d_new)^2 / 2.  d_new: the measured absolute
    error of the device's new neglogp (None: tol (1 + max |neglogp64|))"""
    pol = model.policy
    before = [p.detach().clone() for p in pol.parameters()]
    shuffles = model._shuffles
    want = R.expected_stats(model, batch, rep, CLIPRANGE, shuffles).numpy()
    got = model.update(batch, 0.0, CLIPRANGE).double().cpu().numpy()
    torch.cuda.synchronize()
    for a, b in zip(before, pol.parameters()):
        assert torch.equal(a, b)
    nlp_scale = 1.0 + float(rep["neglogp"].abs().max())
    d_old = float((batch["neglogpacs"].double().cpu() - rep["neglogp"]).abs().max())
    d_new = tol * nlp_scale if d_new is None else d_new
    line = "pg %.2e (want %.2e) vf %.7g (%.7g) entropy %.7g (%.7g) approxkl %.2e (bound %.2e) clipfrac %g" % (
        got[0], want[0], got[1], want[1], got[2], want[2], got[3], 0.5 * (d_old + d_new) ** 2, got[4])
    print(line)
    assert got[4] == 0.0 and want[4] == 0.0, line
    np.testing.assert_allclose(got[:3], want[:3], rtol=10 * tol, atol=tol, err_msg=line)
    assert got[3] <= 0.5 * (d_old + d_new) ** 2, line
    return line


def lstm_zero_lr_check(model, batch, last, prec):
    """the recurrent policy's lr-0 update at the arithmetic `prec` of the sequence kernels (the caller has set lstm_fused.PRECISION): what the
    update's forward pass gives on the device for the recorded batch against float64 within FL.BOUNDS[prec] (`hold`), then `zero_lr_update`
    with the measured error of the new neglogp"""
    pol = model.policy
    assert model.nminibatches == 1 and model.fused_loss and model.fused_heads and pol.fused_heads_supported(batch["obs"])
    rep = R.replay(pol, batch, last)
    # per sample: what the update's forward pass gives on the device for the recorded batch
    nlp, val, _ = pol.evaluate(batch["obs"], batch["states"], batch["masks"], batch["actions"])
    errs = {"neglogp": FL.rel_err(nlp.detach(), rep["neglogp"]), "value": FL.rel_err(val.detach(), rep["value"])}
    print("\n[lr-0 update, lstm, %s, %d robots] evaluate on the device against float64: %s" % (prec, batch["masks"].shape[1], FL.fmt(errs)))

    def fallback():
        r32 = R.replay(pol, batch, last, dtype=torch.float32)
        return {"neglogp": FL.rel_err(r32["neglogp"], rep["neglogp"]), "value": FL.rel_err(r32["value"], rep["value"])}
    hold(("evaluate", prec), errs, {k: FL.BOUNDS[prec] for k in errs}, fallback)
    d_new = float((nlp.detach().double().cpu() - rep["neglogp"]).abs().max())
    # (hence |exp(old - new) - 1| of every sample within expm1 of the two measured errors' sum)
    ratio = torch.exp(batch["neglogpacs"].double().cpu() - nlp.detach().double().cpu())
    print("max |ratio - 1| %.2e" % float((ratio - 1.0).abs().max()), end="  ")
    return zero_lr_update(model, batch, last, rep, FL.BOUNDS[prec], d_new=d_new)
