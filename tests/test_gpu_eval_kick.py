"""The kick table of the device evaluation loop -- caller-specified base-state displacements at chosen control steps (PolicyEvaluator.set_scenario(kicks=)
-> irrl_lstm_eval_perturbed[_persistent], evaluate.perturb_base -> irrl_env_perturb_base[_host]) -- on the MI355X: the kick kernel against the float64
twin, the five-launch form's routing, the two device forms against each other bit for bit, neutrality, the refusals, and the perturbation study's
closed loop against the host-driven twin.

Pool and actor as tests/test_gpu_eval_persistent.py builds them (its helpers are used): bp5_manual_eval.yaml, N = 19 (a last wave of three robots and a
shadow row), D = 6 with delays e % 6, frictions 0.05 .. 0.8, filters at 1 / 50 / 30 Hz, the bp5_155 actor, 60 steps.  The kick table: two rows that fire
at steps 20 and 37 (kick_first 20, kick_every 17; with the scenario of tests/test_gpu_eval_scenario.py, whose t0 is 4: kick_first 16) -- small kicks
(a tenth of the reference's exploration amplitudes) everywhere, sentinel rows (dq = 0, the other words non-zero) on the envs e % 5 == 2, the identity
kick on env 0 in row 0, a roll of 1.5 rad on env 0 in row 1 (its `done` at step 37: the reset path inside the step loop), a real kick on the pool's
last robot in both rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import parity_lib as PL
import test_eval_kick_host as TK
import test_gpu_eval_persistent as TP
import test_gpu_eval_scenario as TS
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.checkpoint import NumpyLstmActor

N, T, T1, HZ, ALL, ACTOR = TP.N, TP.T, TP.T1, TP.HZ, TP.ALL, TP.ACTOR
KICK_FIRST, KICK_EVERY = 20, 17
KICK_STEPS = (KICK_FIRST, KICK_FIRST + KICK_EVERY)
NOISE = dict(z_noise=0.02, roll_noise=0.25, pitch_noise=0.25, z_dot_noise=1.0, roll_dot_noise=1.0, pitch_dot_noise=1.0)      # Exp_Raw_Data/Param-*.txt


@pytest.fixture(scope="module")
def policy():
    return EV.load_policy(ACTOR, torch.device("cuda"))


def _table(n):
    """-> [2, n, 11] float32, see the module's text"""
    rng = np.random.RandomState(11)
    k = EV.kick_rows(dz=rng.uniform(-0.002, 0.002, (2, n)), roll=rng.uniform(-0.03, 0.03, (2, n)), pitch=rng.uniform(-0.03, 0.03, (2, n)),
                     dv=rng.uniform(-0.1, 0.1, (2, n, 3)), dw=rng.uniform(-0.1, 0.1, (2, n, 3)))
    k[:, np.arange(n) % 5 == 2, 1:5] = 0.0
    k[0, 0] = EV.kick_rows()
    k[1, 0] = EV.kick_rows(roll=1.5)
    return k


def _install(ev, scenario):
    if scenario:
        ev.set_scenario(cmd_schedule=TS._table(ev.n), cmd_every=TS.CMD_EVERY, heading=TS._heading(ev.n), stat_buckets=TS.B, stat_every=TS.STAT_EVERY, t0=TS.T0,
                        kicks=_table(ev.n), kick_first=KICK_FIRST - TS.T0, kick_every=KICK_EVERY)
    else:
        ev.set_scenario(kicks=_table(ev.n), kick_first=KICK_FIRST, kick_every=KICK_EVERY)
    return ev


def _run(ev, calls):
    """calls: step counts, or (steps, persistent) pairs"""
    return TP._cat([ev.run(c[0], record=ALL, persistent=c[1]) for c in calls])


def _same(a, b, n):
    TP._assert_same_buffers(a, b, n)
    assert a.stats.shape == b.stats.shape and torch.equal(a.heading_int, b.heading_int)


# ---- 1. the kick kernel against the twin ----
@pytest.mark.parametrize("lanes", [16, 4])
def test_perturb_base_against_the_float64_twin(monkeypatch, lanes):
    """irrl_env_perturb_base (device rows; the 16-lane pool) and irrl_env_perturb_base_host (the 4-lane pool) on the base states and kicks of
    tests/test_eval_kick_host.py: get_state before and after -- z and the quaternion within 2e-6, the velocities within 4e-6 of evaluate.apply_kick;
    every word the kick does not own bit-identical; every env with a sentinel row bit-identical as a whole"""
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", str(lanes))
    env = TP._pool(N)
    assert env.lanes_per_robot == lanes
    base, kick = TK.base_states(31), TK.kick_case(32)
    st = env.get_state()
    st[:, 2:7] = base[:, 0:5]
    st[:, 19:25] = base[:, 5:11]
    env.set_state(st)
    before = env.get_state()
    assert np.array_equal(before[:, 2:7], base[:, 0:5].astype(np.float64)) and np.array_equal(before[:, 19:25], base[:, 5:11].astype(np.float64))
    if lanes == 16:
        EV.perturb_base(env, torch.from_numpy(kick).cuda())
        torch.cuda.synchronize()
    else:
        EV.perturb_base(env, kick)
    after = env.get_state()
    want = EV.apply_kick(before, kick)
    own = np.zeros(288, bool)
    own[2:7] = True
    own[19:25] = True
    err_zq, err_v = np.abs(want[:, 2:7] - after[:, 2:7]).max(), np.abs(want[:, 19:25] - after[:, 19:25]).max()
    print("max |device - apply_kick| (%d lanes): z and quaternion %.3g (bound %.0e), velocities %.3g (bound %.0e)" % (lanes, err_zq, TK.BOUND_ZQ, err_v, TK.BOUND_V))
    assert err_zq <= TK.BOUND_ZQ and err_v <= TK.BOUND_V
    assert np.array_equal(after[:, ~own], before[:, ~own])
    assert TK.SENTINEL.sum() >= 3 and np.array_equal(after[TK.SENTINEL], before[TK.SENTINEL])
    moved = np.abs(after[:, own] - before[:, own]).max(1)
    assert np.all(moved[~TK.SENTINEL][1:] > 1e-3)


# ---- 2. routing, five-launch form ----
def test_five_launch_routing_equals_plain_steps_and_perturb_base(policy):
    """ONE irrl_lstm_eval_perturbed call of 60 steps with the two kick rows == 20 plain steps, irrl_env_perturb_base(row 0), 17 plain steps,
    irrl_env_perturb_base(row 1), 23 plain steps, bit for bit: every recorder, stats, the ring, the histories, lstm_state, get_state, GetJointEffort"""
    a = _install(TP._evaluator(policy, N, **HZ), False)
    ra = _run(a, [(T, False)])
    b = TP._evaluator(policy, N, **HZ)
    rows = torch.from_numpy(_table(N)).cuda()
    parts = [b.run(KICK_FIRST, record=ALL)]
    b.perturb_base(rows[0])
    parts.append(b.run(KICK_EVERY, record=ALL))
    b.perturb_base(rows[1])
    parts.append(b.run(T - KICK_FIRST - KICK_EVERY, record=ALL))
    assert b.scenario is None and a.scenario["kicks"] is not None
    TP._assert_same_records(ra, TP._cat(parts))
    a.stats = a.stats[0]
    TP._assert_same_buffers(a, b, N, full_state=True)
    done = ra["done"].cpu().numpy()
    assert done[KICK_STEPS[1], 0] and not done[:KICK_STEPS[1]].any()          # the roll of 1.5 rad ends env 0's episode on the step it hits


# ---- 3. persistent == five-launch ----
@pytest.fixture(scope="module")
def plain(policy):
    """the 19-env run WITHOUT kicks, five-launch: what the kicked runs are told apart from"""
    ev = TP._evaluator(policy, N, **HZ)
    rec = ev.run(T, record=("body", "done"))
    return {k: v.cpu().numpy() for k, v in rec.items()}


@pytest.mark.parametrize("scenario", [False, True], ids=["kicks", "kicks+scenario"])
@pytest.mark.parametrize("n", [N, 1, 16])
@pytest.mark.parametrize("over, variant", [({}, "shipped_flat"), ({"ContactExit": 0}, "md")])
def test_persistent_equals_five_launch_with_kicks(policy, plain, over, variant, n, scenario):
    """60 steps in the five-launch form against the persistent form issued as 60, as 20 + 40 (a kick on the first step of a call), as 1 + 0 + 59,
    as 21 + 17 + 22 (both kicks on the LAST step of a call) and with the two forms alternating across both kicks (each kick once in either form):
    every recorder and buffer bit for bit, with and without a command schedule + heading hold + buckets.  The table holds sentinel rows, the
    identity kick, the roll that forces `done` on the step it hits, and a kick on the pool's last robot -- each asserted to happen."""
    five = _install(TP._evaluator(policy, n, over, **HZ), scenario)
    ref = _run(five, [(T, False)])
    assert five.env.kernel_variant == variant and five.persistent_supported
    for calls in ([(T, True)], [(T1, True), (T - T1, True)], [(1, True), (0, True), (T - 1, True)], [(21, True), (17, True), (22, True)],
                  [(T1, True), (10, False), (10, True), (20, False)], [(T1, False), (10, True), (10, False), (20, True)]):
        ev = _install(TP._evaluator(policy, n, over, **HZ), scenario)
        TP._assert_same_records(_run(ev, calls), ref)
        _same(ev, five, n)
    # what the table holds, and that it happened
    table = _table(n)
    on = EV.kick_on(table)
    rec = {k: ref[k].cpu().numpy() for k in ("body", "done")}
    assert np.array_equal(table[0, 0], EV.kick_rows()) and on[0, 0] and on[:, n - 1].all()
    assert rec["done"][KICK_STEPS[1], 0] and not rec["done"][:KICK_STEPS[1]].any() and int(rec["done"].sum()) == 1
    if n >= 3:
        assert (~on).any() and np.array_equal(~on[0], np.arange(n) % 5 == 2)
    if n == N and not over and not scenario:
        same = np.all(rec["body"] == plain["body"], axis=2)                       # [T, N]: is the env's body frame the unkicked run's
        assert same[:KICK_FIRST].all()
        assert not same[KICK_FIRST, on[0]][1:].any() and not same[KICK_FIRST, N - 1]   # every kicked env left it at step 20, the last robot too
        # An env with a sentinel row is untouched by the kick itself (test 1 holds that bit for bit), but not by its neighbours': the contact
        # sweeps of a substep end for the whole wave at once, so a kicked robot changes how many sweeps the robots of its wave get -- at the
        # solver's tolerance.  Likewise env 0, whose identity kick only renormalises q.  Both stay far nearer the unkicked run than a kicked env.
        moved = np.abs(rec["body"][KICK_FIRST] - plain["body"][KICK_FIRST]).max(1)
        kicked = on[0].copy()
        kicked[0] = False
        print("step %d, max |body - unkicked body|: sentinel envs %.3g, env 0 (identity kick) %.3g, kicked envs %.3g .. %.3g"
              % (KICK_FIRST, moved[~on[0]].max(), moved[0], moved[kicked].min(), moved[kicked].max()))
        assert moved[~on[0]].max() < np.median(moved[kicked]) and moved[0] < np.median(moved[kicked])
        assert not same[KICK_STEPS[1], 0]


# ---- 4. neutrality ----
@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("scenario", [False, True], ids=["rollout", "scenario"])
def test_null_kicks_and_sentinel_tables_equal_the_old_entry_points(policy, scenario, persistent):
    """the old entry points (irrl_lstm_eval_rollout / _scenario[_persistent]) against irrl_lstm_eval_perturbed[_persistent] with kicks = NULL, and
    against a table of sentinel rows only: records and buffers bit for bit, 20 + 40 with the drop of envs 3 and 17"""
    def build(entry, sentinel=False):
        ev = TP._evaluator(policy, N, **HZ)
        if sentinel:
            k = _table(N)
            k[:, :, 1:5] = 0.0
            k[:, 0, 0], k[:, 0, 5:] = 0.001, 0.05           # (env 0's rows were the identity and the pure roll: give them other words too)
            assert not EV.kick_on(k).any() and np.all(k[:, :, 0] != 0) and np.all(k[:, :, 5:] != 0)
            if scenario:
                ev.set_scenario(cmd_schedule=TS._table(N), cmd_every=TS.CMD_EVERY, heading=TS._heading(N), stat_buckets=TS.B, stat_every=TS.STAT_EVERY,
                                t0=TS.T0, kicks=k, kick_first=KICK_FIRST - TS.T0, kick_every=KICK_EVERY)
            else:
                ev.set_scenario(kicks=k, kick_first=KICK_FIRST, kick_every=KICK_EVERY)
        elif scenario:
            TS._install(ev)
        ev.entry_points = entry
        rec = TS._run(ev, (T1, T - T1), persistent, drop_at=T1)
        if sentinel and not scenario:
            ev.stats = ev.stats[0]              # (set_scenario's one bucket [1, 18, N] against the plain [18, N])
        return ev, rec
    old, r_old = build("auto")
    new, r_new = build("perturbed")
    off, r_off = build("auto", sentinel=True)
    assert (old.scenario is not None) == scenario and (new.scenario is not None) == scenario and off.scenario["kicks"] is not None
    for ev, rec in ((new, r_new), (off, r_off)):
        TP._assert_same_records(r_old, rec)
        _same(old, ev, N)
    assert sorted(np.flatnonzero(r_old["done"].cpu().numpy()[T1])) == TP.FALLERS


# ---- 5. refusals ----
def test_capability_and_refusals_with_kicks(policy):
    """a Crutial pool, a ContactSolver 0 pool and a (32, 32) policy are refused by the persistent kick call with the condition and the new entry
    point named; the five-launch kick call runs on them, and "auto" takes it"""
    from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy
    torch.manual_seed(5)
    small = CustomLSTMPolicy(n_lstm=(32, 32)).to(torch.device("cuda"))
    small.prepare()
    n = 6
    for over, pol, word in (({"Crutial": True}, policy, "crutial"), ({"ContactSolver": 0}, policy, "dir"), ({}, small, "hid 48")):
        a, b = _install(TP._evaluator(pol, n, over, **HZ), False), _install(TP._evaluator(pol, n, over, **HZ), False)
        assert a.persistent_supported is False
        with pytest.raises(RuntimeError, match=word) as info:
            a.run(3, persistent=True)
        assert "irrl_lstm_eval_perturbed_persistent" in str(info.value) and a.t == 0
        ra, rb = a.run(25, record=ALL, persistent="auto"), b.run(25, record=ALL, persistent=False)
        TP._assert_same_records(ra, rb)
        torch.cuda.synchronize()
        assert a.t == 25 and np.array_equal(a.env.get_state(), b.env.get_state())
        bare = TP._evaluator(pol, n, over, **HZ)
        body = bare.run(25, record=("body",))["body"]
        assert torch.equal(body[:KICK_FIRST], ra["body"][:KICK_FIRST]) and not torch.equal(body[KICK_FIRST], ra["body"][KICK_FIRST])


# ---- 6. the closed loop ----
MUS, DELAYS, CMD, E, WARM, FRAMES, BUCKET, SEED, SCALE = (0.8, 0.1), (0, 1), 5.0, 8, 300, 400, 100, 7, 0.1


def test_perturbation_study_agrees_with_the_host_driven_twin():
    """evaluate.perturbation_study -- frictions 0.8 and 0.1 (the Param files') x delays 0, 1 x 8 explorations at 5 m/s, 300 warm-up steps on friction
    0.8, one kick of a tenth of the Param amplitudes (z 0.002 m, roll / pitch 0.025 rad, z / roll / pitch rates 0.1), 400 frames, buckets of 100 steps
    (one gait period), persistent launches -- against evaluate.reference_rollout(kicks=) on HipVecEnv (same GPU) with the same kicks.  No robot falls
    in either loop; per robot, the last bucket's v_x, height and mean pitch lie inside parity_lib.RAISIM_LOG_TOL of the host-driven loop's (2 %,
    4 mm, 0.004 rad); no condition is excluded.
    The kicks were chosen on the CPU oracle before any device run: at this size reference_rollout(kicks=) on the f64 oracle keeps all 32 robots up.
    At step 300 the robots are still accelerating (v_x 1.8 m/s in the bucket in front of the kick, 4.6 - 4.9 m/s in the last one on friction 0.8,
    2.7 - 2.9 m/s on 0.1), so the comparison covers the kick on a transient.  Margin, measured the way the staircase test's was: this twin on the f64
    oracle with N(0, 2e-5) noise on the actions, three seeds against the noise-free run, worst robot per condition, last bucket --
        mu 0.8 delay 0: v_x 2.9e-3 relative, z 2.3e-4 m, pitch 3.5e-4 rad        mu 0.8 delay 1: v_x 1.7e-3, z 3.1e-4 m, pitch 4.9e-4 rad
        mu 0.1 delay 0: v_x 1.5e-3 relative, z 3.7e-4 m, pitch 1.1e-3 rad        mu 0.1 delay 1: v_x 1.5e-3, z 3.2e-4 m, pitch 1.0e-3 rad
    a factor of 3.5 (pitch on friction 0.1) to 13 inside the bounds."""
    from hip_env import HipVecEnv
    conds = [(m, d) for m in MUS for d in DELAYS]
    n = len(conds) * E
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=n)
    noise = {k: SCALE * v for k, v in NOISE.items()}
    rows = EV.perturbation_study(ACTOR, cfg, MUS, DELAYS, CMD, E, noise, warm_steps=WARM, frames=FRAMES, seed=SEED, record_body=True, persistent=True,
                                 bucket_steps=BUCKET)
    kicks = EV.exploration_kicks(n, noise, np.random.default_rng(SEED))
    assert len(rows) == len(conds) and np.array_equal(np.concatenate([r["kicks"] for r in rows]), kicks) and EV.kick_on(kicks).all()
    rec = EV.reference_rollout(HipVecEnv(cfg), NumpyLstmActor.from_npz(ACTOR), cfg, np.repeat([c[1] for c in conds], E), np.full(n, CMD), WARM + FRAMES,
                               mu=np.repeat([c[0] for c in conds], E), warm=WARM, kicks=kicks, kick_first=WARM)
    assert int(rec["falls"].sum()) == 0
    tol = PL.RAISIM_LOG_TOL
    print()
    for i, (c, r) in enumerate(zip(conds, rows)):
        assert (r["mu"], r["delay"], r["cmd"], r["explorations"]) == (c[0], c[1], CMD, E) and r["surviving"] == 1.0 and not r["falls"].any()
        st = r["stats"]
        assert st["frames"].shape == (1 + FRAMES // BUCKET, E) and np.all(st["frames"] == BUCKET) and not st["falls"].any()
        assert r["body"].shape == (FRAMES, E, 13)
        worst = [0.0, 0.0, 0.0]
        for x in range(E):
            e = i * E + x
            # the body log is the post-kick frames, and the kick is visible in its first frame
            h0 = EV.body_statistics(rec["body"][WARM - BUCKET:WARM, e])
            h = EV.body_statistics(rec["body"][WARM + FRAMES - BUCKET:, e])
            d = EV.body_statistics(r["body"][FRAMES - BUCKET:, x])
            assert abs(d["vx_body_mean"] - st["vx_body_mean"][-1, x]) <= 1e-9 and abs(d["z_mean"] - st["z_mean"][-1, x]) <= 1e-9
            assert abs(st["vx_body_mean"][0, x] - h0["vx_body_mean"]) / abs(h0["vx_body_mean"]) < tol["vx_rel"]
            dv = abs(st["vx_body_mean"][-1, x] - h["vx_body_mean"]) / abs(h["vx_body_mean"])
            dz, dp = abs(st["z_mean"][-1, x] - h["z_mean"]), abs(st["pitch_mean"][-1, x] - h["pitch_mean"])
            worst = [max(worst[0], dv), max(worst[1], dz), max(worst[2], dp)]
            assert dv < tol["vx_rel"] and dz < tol["z_abs"] and dp < tol["pitch_mean_abs"], (c, x, dv, dz, dp)
        print("mu %.1f delay %d: last bucket, worst of %d robots |device - host|: vx %.2e relative (vx %.3f m/s), z %.2e m, pitch %.2e rad"
              % (c[0], c[1], E, worst[0], float(st["vx_body_mean"][-1].mean()), worst[1], worst[2]))
