"""The device evaluation loop with MlpPolicy as the actor (evaluate.PolicyEvaluator -> irrl_mlp_eval_measured, and its persistent single-launch form
irrl_mlp_eval_measured_persistent, kernel csrc/env_eval_mlp_kernels.hpp) on the MI355X: the per-step form piece by piece against what already exists
(the policy-step kernel, the numpy conditioning, the float64 action filter, a second pool replaying the applied actions), and the persistent form
bit for bit against the per-step form.

The scene is that of tests/test_gpu_eval_rollout.py / test_gpu_eval_persistent.py: bp5_manual_eval.yaml with N = 19 envs (ragged against the
16-robot workgroup and the 4-robot wave), D = 6 with delays e % 6, commands 0.5 .. 5 m/s, frictions 0.05 .. 0.8, low-passes 1 / 50 / 30 Hz, T = 60
steps issued as 20 + 40, envs 3 and 17 put at 0.14 m between the calls, all recorders, the statistics and the gait recorder on.  The policy is an
MlpPolicy() under torch.manual_seed(SEED), every parameter moved by N(0, 0.05) as in test_fused_mlp_policy_step_matches_eager_step, the action
head scaled by HEAD so that the clip acts on some elements and not on others (asserted on the record)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_eval_persistent as TP
import test_gpu_eval_rollout as TR
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.helper import obs_normalisation
from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import MlpPolicy

N, D, T, T1, HZ, FALLERS = TP.N, TP.D, TP.T, TP.T1, TP.HZ, TP.FALLERS
ALL = TP.ALL + ("gait",)
SEED, HEAD = 7, 12.0
# every column of the work array: both forms write all of them (include/irrl_env.h), `value` and `neglogp` included
WORK = dict(TP.WORK, value=(71, 1), neglogp=(72, 1))
STATE = ("stats", "ring", "cmd", "vel_his", "act_his", "done", "obs", "work", "heading_int", "prev_contact")


def _mlp(seed=SEED, head=HEAD, noise=0.05):
    torch.manual_seed(seed)
    pol = MlpPolicy().to(torch.device("cuda"))
    with torch.no_grad():
        if noise:
            for p in pol.parameters():
                p.add_(torch.randn_like(p) * noise)
        pol.pi.w.mul_(head)
    return pol


@pytest.fixture(scope="module")
def policy():
    return _mlp()


def _evaluator(pol, n, over=None, depth=D, **kw):
    return TP._evaluator(pol, n, over, depth=depth, **kw)


def _same(a, b, n):
    """everything the two forms promise to leave identical (TP._assert_same_buffers without the LSTM state, and with every work column)"""
    torch.cuda.synchronize()
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for k, (c, w) in WORK.items():
        assert torch.equal(a.work.view(-1)[n * c:n * (c + w)], b.work.view(-1)[n * c:n * (c + w)]), k
    assert (a.gait is None) == (b.gait is None) and (a.gait is None or torch.equal(a.gait, b.gait))
    assert a.t == b.t and a.lstm_state is None and b.lstm_state is None
    assert np.array_equal(a.env.get_state(), b.env.get_state())
    assert np.array_equal(TP._effort(a.env, n), TP._effort(b.env, n))


def _scenario(pol, forms, over=None):
    """the 20 + 40 scene; forms: the `persistent` keyword of the two calls"""
    ev = _evaluator(pol, N, over, **HZ)
    ev.measure_gait()
    first = ev.run(T1, record=ALL, persistent=forms[0])
    TP._drop(ev.env)
    return ev, TP._cat([first, ev.run(T - T1, record=ALL, persistent=forms[1])])


@pytest.fixture(scope="module")
def scene(policy):
    """the per-step form's run, in the dictionary test_gpu_eval_rollout's assertions read"""
    env = TR._pool()
    ev = EV.PolicyEvaluator(env, policy, TR.DELAYS, TR.CMDS, depth=D, **HZ)
    ev.measure_gait()
    ob_reset = ev.obs.clone()
    first = ev.run(T1, record=ALL)
    TR._drop(env)
    rec = TR._cat(first, ev.run(T - T1, record=ALL))
    torch.cuda.synchronize()
    out = dict(pol=policy, ev=ev, ob_reset=ob_reset, rec=rec, np={k: v.cpu().numpy() for k, v in rec.items()}, final=env.get_state(),
               effort=TP._effort(env, N), stats=ev.statistics())
    ev2 = EV.PolicyEvaluator(env, policy, TR.DELAYS, TR.CMDS, depth=D, cmd_hz=1.0, vel_hz=None, act_hz=30.0)
    out["ob_reset2"] = ev2.obs.cpu().numpy()
    out["routing"] = {k: v.cpu().numpy() for k, v in ev2.run(15, record=("obs_cond", "obs_raw")).items()}
    return out


def test_the_clip_is_exercised_and_the_dropped_envs_terminate(scene):
    """a condition on the inputs: some recorded clipped actions sit at +-1, some strictly inside; envs 3 and 17 are done at row 20"""
    a = scene["np"]["act_clipped"]
    at, inside = int((np.abs(a) == 1.0).sum()), int((np.abs(a) < 1.0).sum())
    print("clipped actions at +-1: %d, strictly inside: %d of %d" % (at, inside, a.size))
    assert at > 0 and inside > 0 and at + inside == a.size
    done = scene["np"]["done"]
    assert done.shape == (T, N) and set(FALLERS) <= set(np.flatnonzero(done[T1]))
    assert scene["ev"].lstm_state is None and scene["rec"]["gait"].shape == (T, N, 32)


def test_actor_is_the_policy_step_kernel(scene):
    """1. pol.fused_step replayed over the recorded conditioned observations gives rec_act_clipped bit for bit; the last step's action, value and
    neglogp are the work array's columns"""
    pol, rec, ev = scene["pol"], scene["rec"], scene["ev"]
    done = torch.zeros(N, dtype=torch.bool, device=rec["done"].device)
    for t in range(T):
        act, clipped, value, neglogp, _ = pol.fused_step(rec["obs_cond"][t].contiguous(), None, done, noise=None)
        assert torch.equal(clipped, rec["act_clipped"][t]), t
        done = rec["done"][t].contiguous()
    work = lambda k: ev.work.view(-1)[N * WORK[k][0]:N * (WORK[k][0] + WORK[k][1])]
    assert torch.equal(work("action"), act.reshape(-1)) and torch.equal(work("clipped"), clipped.reshape(-1))
    assert torch.equal(work("value"), value) and torch.equal(work("neglogp"), neglogp)


def test_conditioning_delay_routing_and_action_filter(scene):
    """2. the assertions of tests/test_gpu_eval_rollout.py on this scene (the numpy conditioning needs the done rows of every env that fell)"""
    raw, done, cond = scene["np"]["obs_raw"], scene["np"]["done"], scene["np"]["obs_cond"]
    cfg = TR._cfg()
    mean, std, _, _ = obs_normalisation(cfg)
    dt = float(cfg["control_dt"])
    a_cmd, a_vel = EV.lowpass_alpha(dt, HZ["cmd_hz"]), EV.lowpass_alpha(dt, HZ["vel_hz"])
    target = np.stack([TR.CMDS, np.zeros(N), np.zeros(N)], 1)
    st = EV.condition_state(scene["ob_reset"].cpu().numpy(), D)
    worst = [0.0, 0.0]
    for t in range(T):
        o = EV.condition(st, t, scene["ob_reset"].cpu().numpy() if t == 0 else raw[t - 1], TR.DELAYS, target, a_cmd, a_vel, mean[0:3], std[0:3])
        worst = [max(worst[0], np.abs(o[:, 3:] - cond[t, :, 3:]).max()), max(worst[1], np.abs(o[:, 0:3] - cond[t, :, 0:3]).max())]
        st["cmd"][done[t]] = 0.0
    print("max |device - numpy| conditioned observation: elements 3-34 %.3g, command elements %.3g" % tuple(worst))
    assert worst[0] <= 2e-5 and worst[1] <= 2e-4                                         # the LSTM file's bounds
    TR.test_delay_line_routes_bit_for_bit(scene)
    TR.test_action_filter(scene)
    TR.test_recorders_show_the_pool(scene)


def test_env_steps_equal_a_second_pool_replaying_the_applied_actions(scene):
    """3. TR's replay through step_rows with the same set_state after step 20: obs_raw, reward, done and the final pool state bit for bit"""
    TR.test_env_steps_equal_a_second_pool_replaying_the_applied_actions(scene)
    assert set(FALLERS) <= set(np.flatnonzero(scene["np"]["done"][T1]))


@pytest.mark.parametrize("over, variant", [({}, "shipped_flat"), ({"ContactExit": 0}, "md")])
def test_both_forms_are_bit_identical(policy, over, variant):
    """4. persistent against per-step on the scene, for the kernel _l16 and its run-time-solver twin _rt_l16: every recorder (gait included), the
    evaluator's state, every work column, get_state and GetJointEffort; and 20 persistent + 40 per-step and the reverse equal both"""
    b, rb = _scenario(policy, (False, False), over)
    assert b.env.kernel_variant == variant and b.persistent_supported
    done = rb["done"].cpu().numpy()
    assert set(FALLERS) <= set(np.flatnonzero(done[T1]))
    for forms in ((True, True), (True, False), (False, True)):
        a, ra = _scenario(policy, forms, over)
        TP._assert_same_records(ra, rb)
        _same(a, b, N)
    assert torch.equal(a.stats[EV.STAT_SLOTS.index("n")], torch.full((N,), float(T), dtype=torch.float64, device=a.stats.device))
    assert float(a.gait[0, EV.GAIT_SLOTS.index("n")].sum()) == T * N - done.sum()


PAD, MARK = 256, 0x5A


def _fence(ev):
    """move every buffer of the evaluator's state into the middle of a larger one filled with a byte pattern; -> the larger ones"""
    big = {}
    for k in STATE + ("gait",):
        t = getattr(ev, k)
        raw = torch.full((t.numel() * t.element_size() + 2 * PAD,), MARK, dtype=torch.uint8, device=t.device)
        inner = raw[PAD:PAD + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
        inner.copy_(t)
        setattr(ev, k, inner)
        big[k] = raw
    return big


@pytest.mark.parametrize("n", [1, 16, 17])
def test_edges_of_the_grid(policy, n):
    """5. N = 1, 16, 17 (the last workgroup holds one robot) with D = 3, 12 steps, all recorders: both forms bit-identical, and with the
    evaluator's buffers placed inside larger sentinel-filled ones every byte outside stays untouched"""
    evs, recs, bigs = [], [], []
    for persistent in (True, False):
        ev = _evaluator(policy, n, depth=3, **HZ)
        ev.measure_gait()
        bigs.append(_fence(ev))
        recs.append(ev.run(12, record=ALL, persistent=persistent))
        evs.append(ev)
    TP._assert_same_records(recs[0], recs[1])
    _same(evs[0], evs[1], n)
    for big in bigs:
        for k, raw in big.items():
            assert bool((raw[:PAD] == MARK).all()) and bool((raw[-PAD:] == MARK).all()), k


def test_scenario_kicks_and_gait_sums(policy):
    """6. 48 steps at N = 19 with a 3-row command schedule (cmd_every 16), the heading hold on the odd envs, 3 statistics buckets, one kick row at
    step 10 on envs 0, 5, 18 and gait=True: both forms bit-identical, heading_int, gait, prev_contact and the bucketed stats included"""
    steps = 48
    table = np.stack([(r + 1) / 3.0 * np.linspace(0.5, 5.0, N)[:, None] * np.array([1.0, 0.1, -0.05])[None] for r in range(3)], 0)
    odd = np.arange(N) % 2 == 1
    heading = dict(ref=np.linspace(-0.8, 0.8, N), kp=np.where(odd, 1.0, 0.0), ki=np.where(odd, 0.1, 0.0), windup=0.004)
    kicks = np.zeros((N, EV.KICK_DIM), np.float32)
    kicks[[0, 5, 18]] = EV.kick_rows(dz=0.01, roll=0.2, pitch=-0.15, dv=(0.3, -0.2, 0.5), dw=(0.5, 0.5, -0.5))
    assert sorted(np.flatnonzero(EV.kick_on(kicks))) == [0, 5, 18]
    out = []
    for persistent in (True, False):
        ev = _evaluator(policy, N, **HZ)
        ev.set_scenario(cmd_schedule=table, cmd_every=16, heading=heading, stat_buckets=3, stat_every=16, kicks=kicks, kick_first=10, gait=True)
        out.append((ev, ev.run(steps, record=ALL, persistent=persistent)))
    (a, ra), (b, rb) = out
    TP._assert_same_records(ra, rb)
    _same(a, b, N)
    assert a.stats.shape == (3, len(EV.STAT_SLOTS), N) and a.gait.shape == (3, len(EV.GAIT_SLOTS), N)
    assert torch.equal(a.stats[:, EV.STAT_SLOTS.index("n")].sum(0), torch.full((N,), float(steps), dtype=torch.float64, device=a.stats.device))
    assert bool((a.stats[:, EV.STAT_SLOTS.index("n")].sum(1) > 0).all())                         # every bucket got frames
    hi = a.heading_int.cpu().numpy()
    assert np.all(hi[~odd] == 0.0) and np.any(hi[odd] != 0.0)
    # the kick fired at step 10 and not before: the kicked envs' body rows against a run without the kick table
    ev = _evaluator(policy, N, **HZ)
    ev.set_scenario(cmd_schedule=table, cmd_every=16, heading=heading, stat_buckets=3, stat_every=16, gait=True)
    plain = ev.run(11, record=("body",), persistent=False)["body"]
    moved = (plain[10] != ra["body"][10]).any(1).cpu().numpy()
    assert torch.equal(plain[:10], ra["body"][:10]) and moved[[0, 5, 18]].all()


def test_where_the_persistent_kernel_does_not_exist(policy, monkeypatch):
    """7. a Crutial pool and a 4-lane pool: persistent_supported is False, persistent=True raises with the entry point's name and the condition,
    nothing has run, and "auto" runs the per-step form"""
    n = 6
    for over, lanes, word in (({"Crutial": True}, None, "crutial"), ({}, "4", "16-lane layout")):
        if lanes:
            monkeypatch.setenv("IRRL_LANES_PER_ROBOT", lanes)
        a, b = _evaluator(policy, n, over, **HZ), _evaluator(policy, n, over, **HZ)
        assert a.persistent_supported is False and a.auto_persistent is False
        assert a.env.lanes_per_robot == (4 if lanes else 16)
        with pytest.raises(RuntimeError, match=word) as info:
            a.run(3, persistent=True)
        assert "irrl_mlp_eval_measured_persistent" in str(info.value) and a.t == 0
        ra, rb = a.run(8, record=ALL, persistent="auto"), b.run(8, record=ALL, persistent=False)
        TP._assert_same_records(ra, rb)
        _same(a, b, n)
    with pytest.raises(ValueError, match="entry_points"):
        a.entry_points = "perturbed"
        a.run(1)


def test_robustness_sweep_with_an_mlp_policy():
    """8. robustness_sweep with an MlpPolicy on frictions 0.8 / 0.1 x delays 0 / 3 at 2 m/s, 100 warm-up + 128 steps, gait, footfall and
    recurrence (128 frames) on: the rows are finite, have the keys of the LSTM policy's sweep, and persistent "on" and "off" give identical rows.
    The policy is MlpPolicy() as initialised under SEED with the action head scaled by 30: its robots stay up and drift at 0.14 .. 0.17 m/s in
    every row (measured), above the 0.05 m/s under which a cost of transport is NaN by design -- a condition on the inputs, like the clip's"""
    pol = _mlp(head=30.0, noise=0.0)
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=4)
    kw = dict(warm_steps=100, steps=128, gait=True, footfall=EV.FOOTFALL_SPEC_REFERENCE, recurrence=EV.RECURRENCE_SPEC_REFERENCE, recurrence_frames=128)
    sweep = lambda p, persistent: EV.robustness_sweep(p, cfg, [0.8, 0.1], [0, 3], [2.0], persistent=persistent, **kw)
    on, off, lstm = sweep(pol, "on"), sweep(pol, "off"), sweep(TP.ACTOR, "auto")
    print(EV.sweep_table(on, gait=True, recurrence=True, footfall=True))

    def same(x, y, path):
        if isinstance(x, dict):
            assert sorted(x) == sorted(y), path
            for k in x:
                same(x[k], y[k], path + (k,))
        elif isinstance(x, np.ndarray):
            assert x.tobytes() == y.tobytes(), path
        else:
            assert x == y or (x != x and y != y), (path, x, y)
    assert len(on) == len(off) == len(lstm) == 4
    for r_on, r_off, r_lstm in zip(on, off, lstm):
        same(r_on, r_off, ())
        assert sorted(r_on) == sorted(r_lstm)
        assert (r_on["mu"], r_on["delay"], r_on["cmd"]) == (r_lstm["mu"], r_lstm["delay"], r_lstm["cmd"]) and r_on["frames"] == 128
        assert r_on["falls"] == 0 and abs(r_on["vx_body_mean"]) >= 2 * EV.COT_VX_FLOOR
        for k, v in r_on.items():
            if isinstance(v, (int, float)):
                assert np.isfinite(v), (k, v)


def test_the_lstm_forms_are_untouched():
    """9. one short LSTM run, 12 steps at N = 5, through the unchanged entry points: its two forms still leave the same buffers (the launcher
    code they share with the new entry points)"""
    pol = EV.load_policy(TP.ACTOR, torch.device("cuda"))
    a, b = TP._evaluator(pol, 5, **HZ), TP._evaluator(pol, 5, **HZ)
    ra, rb = a.run(12, record=TP.ALL, persistent=True), b.run(12, record=TP.ALL, persistent=False)
    TP._assert_same_records(ra, rb)
    TP._assert_same_buffers(a, b, 5)
    assert a.lstm_state is not None and a.is_mlp is False
