"""Shared pieces of tests/test_rollout_replay_reference.py (CPU) and tests/test_gpu_rollout_replay.py (MI355X): the float64 replay of a
recorded rollout.  A rollout hands the update `obs`, `actions`, `neglogpacs`, `values`, `masks`, `states`, `true_reward` and `returns`; the
update takes them for the old policy's numbers on exactly those samples.  Everything here recomputes those numbers from the recorded
OBSERVATIONS alone, with code that shares nothing with the rollout kernels:

  sampler_reference   the exploration noise of (seed, global env id, global step, action slot): Philox4x32-10 + Box-Muller in numpy float64
  replay              ONE eager `_run` over the whole [T, N] batch on a float64 copy of the policy, from batch["states"] and batch["masks"]
                      -> mean, values, final state, neglogp of the recorded actions, and the bootstrap value
  capture_value_call  what the runner handed to `policy.value` after the last step (it overwrites its `obs` with env.reset() before it returns)
  gae64               ppo2.gae_reference on float64 copies
  expected_stats      ppo2.ppo_loss in float64 on the replayed numbers, minibatch by minibatch as `update` cuts and averages them
  ballistic_ends      the scenario: chosen robots are thrown upwards so that their episode ends in a chosen row of the rollout

Conventions under test (ppo2.Runner): masks[t] is the done flag IN FRONT OF step t; `states` is the state in front of the rollout, before
masks[0] is applied; the state is [c | h] per layer, actor stack then critic stack; reward row t is the reward of step t; the bootstrap is
V(observation after the last step, carried state, dones after the last step).
"""
import contextlib
import copy
import math
import os
import sys

import numpy as np
import torch

from conftest import ROOT
from high_speed_quadrupedal_locomotion_by_irrl_amd import ppo2 as P2
from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import SBLstm, diag_gaussian_neglogp

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_actions import philox4x32_10  # noqa: E402

import lstm_forms_lib as FL  # noqa: E402
import oracle as O  # noqa: E402

POLICY_NOISE_KEY = 0x49525231       # 'IRR1': the engine's Philox key word
POLICY_NOISE_PURPOSE = 0x50         # purpose word of the sampling noise: action slots 4 q .. 4 q + 3 use 0x50 + q

T_STEPS, N_ENVS, ENV_ID_OFFSET = 24, 40, 1000
GAMMA, LAM = 0.99, 0.95


# ---- the sampler ----
def sampler_uniforms(seed, env_ids, gsteps, block):
    """the four uniforms u = (word >> 8) / 2^24 of counter (env id mod 2^32, gstep >> 32, gstep & 0xffffffff, 0x50 + block), key (seed, 'IRR1');
    env_ids, gsteps, block broadcast -> float64 [..., 4]"""
    env = np.asarray(env_ids, np.int64) & 0xFFFFFFFF
    g = np.asarray(gsteps, np.int64)
    words = philox4x32_10(env.astype(np.uint32), ((g >> 32) & 0xFFFFFFFF).astype(np.uint32), (g & 0xFFFFFFFF).astype(np.uint32),
                          (POLICY_NOISE_PURPOSE + np.asarray(block, np.int64)).astype(np.uint32), int(seed) & 0xFFFFFFFF, POLICY_NOISE_KEY)
    return np.stack([(w >> np.uint32(8)).astype(np.float64) / 16777216.0 for w in words], -1)


def box_muller(u, swap_pairs=False):
    """[..., 4] uniforms -> [..., 4] standard normals: (u0, u1) gives slots 0 (cos) and 1 (sin), (u2, u3) slots 2 and 3; r = sqrt(-2 ln(1 - u_a)),
    angle 2 pi u_b.  swap_pairs: the two pairs exchanged (a negative control)"""
    pairs = ((2, 3), (0, 1)) if swap_pairs else ((0, 1), (2, 3))
    out = []
    for a, b in pairs:
        r = np.sqrt(-2.0 * np.log(1.0 - u[..., a]))
        out += [r * np.cos(2.0 * np.pi * u[..., b]), r * np.sin(2.0 * np.pi * u[..., b])]
    return np.stack(out, -1)


def sampler_reference(seed, env_ids, gsteps, act_dim=12, swap_pairs=False):
    """Standard normals the policy kernels draw for GLOBAL env ids `env_ids` at global steps `gsteps` (= rng_step + row + rng_base); the two
    broadcast against each other -> float64 [..., act_dim]"""
    env, g = np.broadcast_arrays(np.asarray(env_ids, np.int64), np.asarray(gsteps, np.int64))
    blocks = (act_dim + 3) // 4
    u = sampler_uniforms(seed, env[..., None], g[..., None], np.arange(blocks))          # [..., blocks, 4]
    z = box_muller(u, swap_pairs)
    return z.reshape(z.shape[:-2] + (4 * blocks,))[..., :act_dim]


# ---- the replay ----
@contextlib.contextmanager
def capture_value_call(policy):
    """Within the block every `policy.value(obs, states, dones)` is passed on and noted as {obs, states, dones, result} (clones): the one
    call inside Runner.run() is the bootstrap"""
    calls, inner = [], policy.value

    def value(obs, states=None, masks=None):
        out = inner(obs, states, masks)
        calls.append({"obs": obs.clone(), "states": None if states is None else states.clone(), "dones": masks.clone(), "result": out.clone()})
        return out
    policy.value = value
    try:
        yield calls
    finally:
        del policy.value


def clone_batch(batch):
    """the runner hands out its own buffers, which the next rollout overwrites"""
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}


def replay(policy, batch, last, dtype=torch.float64, masks=None):
    """One eager `_run` over the whole recorded batch on a copy of the policy in `dtype` on the CPU -> {mean [T, N, A], value [T, N], neglogp
    [T, N] of the recorded actions, state [N, S] after the last row (None for a policy without one), last_value [N] from that state and the
    captured last observation / dones}.  masks: replaces batch["masks"] (the power checks)."""
    p = copy.deepcopy(policy).to(device="cpu", dtype=dtype)
    cast = lambda t: t.detach().to(device="cpu", dtype=dtype)
    obs, actions = cast(batch["obs"]), cast(batch["actions"])
    m = cast(batch["masks"] if masks is None else masks)
    try:
        SBLstm.use_fused = False
        with torch.no_grad():
            if policy.recurrent:
                mean, value, state = p._run(obs, cast(batch["states"]), m)
                last_value = p._run(cast(last["obs"]).unsqueeze(0), state, cast(last["dones"]).unsqueeze(0))[1][0]
            else:
                mean, value = p._run(obs)
                state, last_value = None, p._run(cast(last["obs"]))[1]
            return {"mean": mean, "value": value, "state": state, "neglogp": diag_gaussian_neglogp(actions, mean, p.logstd), "last_value": last_value,
                    "logstd": p.logstd.detach().clone()}
    finally:
        SBLstm.use_fused = True


def shifted_masks(batch, last):
    """masks one row early: row t holds the flag of row t + 1, the last row the flag after the last step"""
    m = batch["masks"]
    return torch.cat([m[1:], last["dones"].to(m.dtype).unsqueeze(0)], 0)


def ended_envs(batch, last):
    """robots with an episode end inside the rollout or after its last step (rows 1 .. T)"""
    return (batch["masks"][1:].any(0) | last["dones"].bool()).cpu()


def gae64(rewards, values, masks, last_values, last_dones, gamma=GAMMA, lam=LAM):
    """ppo2.gae_reference on float64 copies -> advantages, returns"""
    d = lambda t: t.detach().to(device="cpu", dtype=torch.float64)
    return P2.gae_reference(d(rewards), d(values), d(masks), d(last_values), d(last_dones), gamma, lam)


def minibatch_partition(model, T, N, shuffles):
    """the minibatches of one `update` as index vectors into the flat [T * N] batch (t * N + env), in the order `update` takes them.  A
    recurrent policy with one minibatch takes the whole batch noptepochs times; a non-recurrent one cuts the keyed permutation
    ppo2.feistel_permutation(n, key, shuffle count) -- `_sample_order`'s -- of every epoch.  shuffles: model._shuffles in front of the update."""
    n = T * N
    if model.policy.recurrent:
        assert model.nminibatches == 1
        return [np.arange(n)] * model.noptepochs
    key = (model.seed * 1000003 + 12345) & 0xFFFFFFFF
    bs = n // model.nminibatches
    parts = []
    for epoch in range(model.noptepochs):
        order = P2.feistel_permutation(n, key, shuffles + epoch + 1)
        parts += [order[s:s + bs] for s in range(0, n, bs)]
    return parts


def expected_stats(model, batch, rep, cliprange, shuffles):
    """[pg, vf, entropy, approxkl, clipfrac] `model.update(batch, lr, cliprange)` logs while the weights are the rollout's: ppo2.ppo_loss in
    float64 on the REPLAYED neglogp / values / entropy against the RECORDED old ones, advantages normalised per minibatch
    ((A - mean) / (std + 1e-8), population std), averaged over the minibatches as `update` averages"""
    d = lambda t: t.detach().to(device="cpu", dtype=torch.float64).reshape(-1)
    T, N = batch["values"].shape
    ret, ov, onlp = d(batch["returns"]), d(batch["values"]), d(batch["neglogpacs"])
    nlp, v = rep["neglogp"].reshape(-1), rep["value"].reshape(-1)
    ent = (rep["logstd"] + 0.5 * (math.log(2.0 * math.pi) + 1.0)).sum(-1).expand(T * N)
    rows = []
    for part in minibatch_partition(model, T, N, shuffles):
        i = torch.from_numpy(np.asarray(part))
        adv = ret[i] - ov[i]
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
        out = P2.ppo_loss(nlp[i], v[i], ent[i], None, adv, ret[i], onlp[i], ov[i], cliprange, model.ent_coef, model.vf_coef)
        rows.append(torch.stack(out[1:]))
    return torch.stack(rows).mean(0)


# ---- the scenario ----
# designed end row k of a robot: its done flag is raised by the k-th env step of the rollout, so masks[k] is set (k = T: the flag after the last step,
# `last_dones`).  Rows 1, an interior row, T - 1 and T; robots of all three 16-robot workgroups of a 40-robot pool, 33 and 39 in the ragged one.
PLAN = {0: 1, 5: 2, 17: 5, 20: 11, 33: 17, 39: 23, 16: 24}
BALLISTIC_Z0, BALLISTIC_GAP, GRAVITY, BALLISTIC_TRUNK_MASS = 0.60, 0.05, 9.81, 400.0


def ballistic_ends(state, plan, control_dt):
    """-> a copy of the flat pool state [N, 288] in which robot i of `plan` = {i: k} stands still in the air at base height 0.60 m with an upward
    base velocity that carries it over the 0.65 m termination bound in the middle of env step k: 0.05 = vz tau - g tau^2 / 2 at tau = (k - 1/2) dt.
    The toes are 0.2 m above the ground, so nothing acts on the base but gravity and the reaction of the swinging legs.  That reaction is what the
    formula alone cannot be tuned for: the four legs weigh 5.3 kg against a trunk of 3.7 kg and follow the SAMPLED actions (+-1 rad targets), which
    moves the base by up to a centimetre within 24 steps -- five rows at the 1.7 mm per step of the slowest throw, in a direction that depends on
    the noise draw.  The thrown robots therefore get a trunk of 400 kg (the pool state carries the link masses; free flight does not depend on the
    mass): the legs' share of the mass, and with it the base's answer to them, drops to 1.3 %.  The trunk still TURNS under the legs' torques
    (its inertia is the model's), by up to 6 degrees, and the base frame's origin rides on the trunk's centre of mass at a lever of a centimetre
    or two: another 1.5 mm.  So the trunk's centre of mass is put into the origin of its frame.  What is left, measured on the oracle over
    random clipped actions: the base within 0.12 mm of the parabola at every step, against the half step of 0.85 mm of the slowest throw.
    The trunk stays heavy after the in-step reset (it would sink below 0.15 m some 80 steps later: not within these rollouts).  Every other robot
    of the pool is left as it is."""
    st = np.array(state, np.float64, copy=True)
    gc, gv = O.S["GC"], O.S["GV"]
    for i, k in plan.items():
        tau = (k - 0.5) * control_dt
        st[i, gc + 2] = BALLISTIC_Z0
        st[i, gv:gv + 18] = 0.0
        st[i, gv + 2] = BALLISTIC_GAP / tau + 0.5 * GRAVITY * tau
        st[i, O.S["MASS"]] = BALLISTIC_TRUNK_MASS
        st[i, O.S["COM"]:O.S["COM"] + 3] = 0.0
    return st


def apply_plan(runner, plan, control_dt):
    """`ballistic_ends` through get_state / set_state of the runner's pool, then the runner's observation refreshed from the pool: both in front
    of EVERY run(), because the runner resets the pool after a rollout"""
    env = runner.env
    if hasattr(env, "wrapper"):                      # TorchVecEnv over the C-ABI pool
        torch.cuda.synchronize()
        env.wrapper.set_state(ballistic_ends(env.wrapper.get_state(), plan, control_dt))
        env.wrapper.observe(runner.obs)
        torch.cuda.synchronize()
    else:                                            # OracleTorchEnv
        env.env.set_state(ballistic_ends(env.env.get_state(), plan, control_dt))
        runner.obs.copy_(torch.from_numpy(env.env.observe()))


def realised_ends(batch, last):
    """{robot: [rows]} of every done flag raised inside the rollout (rows 1 .. T - 1 of `masks`) or after its last step (row T)"""
    m = batch["masks"][1:].cpu().numpy().astype(bool)
    ld = last["dones"].cpu().numpy().astype(bool)
    out = {}
    for t, i in zip(*np.nonzero(np.concatenate([m, ld[None]], 0))):
        out.setdefault(int(i), []).append(int(t) + 1)
    return out


def perturb_(policy, seed, logstd_range=None):
    """the policy away from its initial point: every parameter but logstd + 0.05 randn; logstd stays 0, or with logstd_range = (lo, hi) is spread
    evenly over it, the slots in a shuffled order"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in policy.parameters():
            if p is not policy.logstd:
                p.add_((torch.randn(p.shape, generator=g) * 0.05).to(p.device))
        if logstd_range is not None:
            lo, hi = logstd_range
            policy.logstd.copy_(torch.linspace(lo, hi, policy.logstd.numel()).reshape(policy.logstd.shape)[:, torch.randperm(policy.logstd.numel(), generator=g)])
    return policy


# ---- a case: model, runner, two consecutive rollouts under the scenario ----
def collect(runner, plan, control_dt, rollouts=2):
    """-> [(batch, last, rng_base)] of `rollouts` consecutive run() calls, the scenario applied in front of each: clones of the recorded batch,
    what the bootstrap call was handed, and the policy steps of all earlier rollouts as the runner counted them in front of the rollout"""
    out = []
    for _ in range(rollouts):
        apply_plan(runner, plan, control_dt)
        base = int(runner.rng_base)
        with capture_value_call(runner.model.policy) as calls:
            batch = clone_batch(runner.run())
        assert len(calls) == 1, len(calls)
        out.append((batch, calls[0], base))
    return out


REPLAY_TOL = {"value": FL.STEP_TOL["value"], "neglogp": FL.STEP_TOL["neglogp"], "state_pi": FL.STEP_TOL["state"], "state_v": FL.STEP_TOL["state"],
              "last_value": FL.STEP_TOL["value"]}
RETURNS_TOL = 2e-5          # x (1 + max |returns|): the project's f32 level for values and returns
POWER = 100.0


def replay_errors(policy, batch, last, rep):
    """lstm_forms_lib.step_errors (|recorded - replayed| max / (1 + max |replayed|)) of what the rollout recorded and what it handed to the
    bootstrap call: values, neglogp, the carried state by halves (actor stack | critic stack), the bootstrap value"""
    out = {"value": batch["values"], "neglogp": batch["neglogpacs"], "last_value": last["result"]}
    ref = {"value": rep["value"], "neglogp": rep["neglogp"], "last_value": rep["last_value"]}
    if policy.recurrent:
        half = policy.state_dim // 2
        out.update(state_pi=last["states"][:, :half], state_v=last["states"][:, half:])
        ref.update(state_pi=rep["state"][:, :half], state_v=rep["state"][:, half:])
    return FL.step_errors(out, ref)


def returns_errors(batch, last, rep):
    """recorded returns and returns - values against gae64 of the recorded f32 rewards / values / masks and the REPLAYED bootstrap value,
    max |.| / (1 + max |returns64|)"""
    adv, ret = gae64(batch["true_reward"], batch["values"], batch["masks"], rep["last_value"], last["dones"])
    scale = 1.0 + float(ret.abs().max())
    r, v = batch["returns"].double().cpu(), batch["values"].double().cpu()
    return {"returns": float((r - ret).abs().max()) / scale, "advantages": float((r - v - adv).abs().max()) / scale}


def power_errors(policy, batch, last, rep):
    """The same checks with `masks` one row early (`shifted_masks`), per robot whose episode ended: the error of the recorded values against
    that replay (recurrent policies: the masks clear the state) and of the recorded returns against gae64 over those masks, in the metrics of
    `replay_errors` / `returns_errors` -> {robot: (value error or None, returns error)}"""
    sm = shifted_masks(batch, last)
    adv, ret = gae64(batch["true_reward"], batch["values"], sm, rep["last_value"], torch.zeros_like(last["dones"]))
    r_err = (batch["returns"].double().cpu() - ret).abs().amax(0) / (1.0 + float(ret.abs().max()))
    v_err = None
    if policy.recurrent:
        bad = replay(policy, batch, last, masks=sm)
        v_err = (batch["values"].double().cpu() - bad["value"]).abs().amax(0) / (1.0 + float(rep["value"].abs().max()))
    return {int(i): (None if v_err is None else float(v_err[i]), float(r_err[i])) for i in torch.nonzero(ended_envs(batch, last)).reshape(-1)}


def sampler_error(model, batch, rep, rng_base):
    """max |z - sampler_reference| over every row, env and slot, z = (recorded action - replayed mean) / exp(logstd)"""
    T, N, A = batch["actions"].shape
    z = (batch["actions"].double().cpu() - rep["mean"]) / torch.exp(rep["logstd"])
    want = sampler_reference(model.noise_seed, (np.arange(N) + model.env_id_offset)[None, :], (np.arange(T) + rng_base)[:, None], A)
    return float(np.abs(z.numpy() - want).max())
