"""The gait measurements of the device evaluation loop -- joint power, torque and ground-force sums and the footfall pattern at control-step rate
(PolicyEvaluator.set_scenario(gait=True) / measure_gait / run(record=("gait",)) -> irrl_lstm_eval_measured[_persistent]) -- on the MI355X: the two
device forms against each other bit for bit, the device sums against the numpy twin of the recorder's rows, the recorder against the pool,
neutrality of a NULL struct and of the recorder alone, the refusals, and the closed loop against the host-driven twin.

Pool and actor as tests/test_gpu_eval_persistent.py builds them (its helpers are used): bp5_manual_eval.yaml, D = 6 with delays e % 6, frictions
0.05 .. 0.8, filters at 1 / 50 / 30 Hz, the bp5_155 actor, 60 control steps from the reset drop, pools of n = 1 (one robot), 16 (one full workgroup)
and 22 (a last wave of two robots beside idle rows).  Three buckets of 25 steps (boundaries inside the call; with the scenario of
tests/test_gpu_eval_scenario.py, whose t0 is 4, at steps 29 and 54).  The kick table of tests/test_gpu_eval_kick.py on another schedule: small kicks at
step 20 and a roll of 1.5 rad on env 0 at step 50, whose episode ends on that step -- behind the landing of the reset drop, which the CPU oracle puts at
steps 42 .. 45 for every robot of these pools, so that env 0 too has a touchdown in front of its `done`.  Both are asserted: without them the tests
are vacuous.
Rows compared with the twin bit for bit / to 1e-12 relative as tests/test_eval_gait_host.py states; the recorder holds only the z component of the
impulses, so the twin has no peak_grf row (the two device forms are held to each other on it, and the host program to the twin with lamw given)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_eval_gait_host as TG
import test_gpu_eval_kick as TK
import test_gpu_eval_persistent as TP
import test_gpu_eval_scenario as TS
from conftest import load_env_cfg
from high_speed_quadrupedal_locomotion_by_irrl_amd import evaluate as EV
from high_speed_quadrupedal_locomotion_by_irrl_amd.checkpoint import NumpyLstmActor

T, HZ, ACTOR = TP.T, TP.HZ, TP.ACTOR
ALL = TP.ALL + ("gait",)
SIZES = [22, 1, 16]
BUCKETS, STAT_EVERY = 3, 25
KICK_FIRST, KICK_EVERY = 20, 30
TIP_STEP = KICK_FIRST + KICK_EVERY
G = TG.G


@pytest.fixture(scope="module")
def policy():
    return EV.load_policy(ACTOR, torch.device("cuda"))


def _install(ev, scenario, gait=True):
    """the kick table, three buckets of 25 steps and the gait measurements; scenario: the command schedule and heading hold of the scenario tests too"""
    if scenario:
        ev.set_scenario(cmd_schedule=TS._table(ev.n), cmd_every=TS.CMD_EVERY, heading=TS._heading(ev.n), stat_buckets=BUCKETS, stat_every=STAT_EVERY, t0=TS.T0,
                        kicks=TK._table(ev.n), kick_first=KICK_FIRST - TS.T0, kick_every=KICK_EVERY, gait=gait)
    else:
        ev.set_scenario(stat_buckets=BUCKETS, stat_every=STAT_EVERY, kicks=TK._table(ev.n), kick_first=KICK_FIRST, kick_every=KICK_EVERY, gait=gait)
    return ev


def _run(ev, calls, record=ALL):
    return TP._cat([ev.run(c[0], record=record, persistent=c[1]) for c in calls])


def _same(a, b, n):
    TP._assert_same_buffers(a, b, n)
    assert a.stats.shape == b.stats.shape and torch.equal(a.heading_int, b.heading_int)
    assert (a.gait is None) == (b.gait is None) and torch.equal(a.prev_contact, b.prev_contact)
    if a.gait is not None:
        assert a.gait.shape == b.gait.shape and torch.equal(a.gait, b.gait)


def _not_vacuous(ev, rec):
    done, gait = rec["done"].cpu().numpy(), ev.gait.cpu().numpy()
    assert done[TIP_STEP, 0] and not done[:TIP_STEP].any()
    assert gait[:, G["touchdown0"]:G["touchdown0"] + 4, 0].sum() >= 1 and gait[:, G["n"]].sum() == done.size - done.sum()
    assert (gait[:, G["n"]].sum(1) > 0).all()                    # every bucket got frames


def _against_the_twin(ev, rec, t0):
    want, prev = EV.gait_rows_numpy(rec["gait"].cpu().numpy(), rec["done"].cpu().numpy(), stat_buckets=BUCKETS, stat_every=STAT_EVERY, t=0, t0=t0)
    TG.compare_rows(ev.gait.cpu().numpy(), want, "device sums against the twin", skip=("peak_grf",))
    assert np.array_equal(ev.prev_contact.cpu().numpy(), prev)
    grf = ev.gait.cpu().numpy()[:, G["peak_grf"]]
    assert np.all(grf >= 0) and grf.max() > 0
    # the peak of the norm is at least the peak of its z component, which the recorder holds
    r = rec["gait"].cpu().numpy()
    live = ~rec["done"].cpu().numpy().astype(bool)
    assert np.all(grf.max(0) >= np.where(live[..., None], np.abs(r[:, :, 28:32]) * (r[:, :, 24:28] != 0), 0).max((0, 2)) * (1 - 1e-6))


# ---- 1. persistent == five-launch ----
@pytest.mark.parametrize("scenario", [False, True], ids=["kicks", "kicks+scenario"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("over, variant", [({}, "shipped_flat"), ({"ContactExit": 0}, "md")])
def test_persistent_equals_five_launch_with_gait(policy, over, variant, n, scenario):
    """60 steps in the five-launch form against the persistent form issued as 60 and as 35 + 25 (sums, prev_contact and the bucket carried across
    calls): gait, prev_contact, rec_gait, every older recorder and buffer and the pool bit for bit; and test 2 for both forms: the device sums
    against the twin of the recorder's rows"""
    five = _install(TP._evaluator(policy, n, over, **HZ), scenario)
    ref = _run(five, [(T, False)])
    assert five.env.kernel_variant == variant and five.persistent_supported and five.gait.shape == (BUCKETS, 20, n)
    _not_vacuous(five, ref)
    _against_the_twin(five, ref, TS.T0 if scenario else 0)
    for calls in ([(T, True)], [(35, True), (25, True)]):
        ev = _install(TP._evaluator(policy, n, over, **HZ), scenario)
        rec = _run(ev, calls)
        TP._assert_same_records(rec, ref)
        _same(ev, five, n)
    _against_the_twin(ev, rec, TS.T0 if scenario else 0)


# ---- 2. the five-launch form in both lane layouts against the twin; 3. the recorder against the pool ----
@pytest.mark.parametrize("lanes", [16, 4])
def test_device_sums_equal_the_twin_and_the_recorder_equals_the_pool(policy, monkeypatch, lanes):
    """irrl_lstm_eval_measured on a 16-lane and on a 4-lane pool of 22: the sums against evaluate.gait_rows_numpy(rec_gait, rec_done); the last
    row of rec_gait is what the pool holds after the call: GetJointEffort | OriginState[:, 25:37] | OriginState[:, 37:41], and lam_w_z / control_dt
    out of get_state"""
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", str(lanes))
    n = 22
    ev = _install(TP._evaluator(policy, n, **HZ), False)
    assert ev.env.lanes_per_robot == lanes
    rec = _run(ev, [(T, False)])
    _not_vacuous(ev, rec)
    _against_the_twin(ev, rec, 0)
    last = rec["gait"][-1].cpu().numpy()
    origin = np.zeros((n, 41), np.float32)
    ev.env.OriginState(origin)
    assert np.array_equal(last[:, 0:12], TP._effort(ev.env, n)) and np.array_equal(last[:, 0:12], rec["torque"][-1].cpu().numpy())
    assert np.array_equal(last[:, 12:24], origin[:, 25:37]) and np.array_equal(last[:, 24:28], origin[:, 37:41])
    st = ev.env.get_state()
    inv_dt = np.float32(1.0) / np.float32(ev.env.cfg_value("control_dt"))
    assert np.allclose(last[:, 28:32], st[:, 137:147:3].astype(np.float32) * inv_dt, rtol=3e-7, atol=0) and last[:, 24:28].any()
    assert np.all(last[:, 28:32][last[:, 24:28] == 0] == 0)          # no impulse on a leg that is not in the contact list


# ---- 4. neutrality ----
@pytest.mark.parametrize("persistent", [False, True])
@pytest.mark.parametrize("mode", ["rollout", "scenario", "kicks"])
def test_null_gait_and_the_recorder_alone_equal_the_old_entry_points(policy, mode, persistent):
    """the old entry points against irrl_lstm_eval_measured[_persistent] with gait = NULL, against the recorder alone (prev_contact NULL), and
    against the full measurements: every older record and buffer and the pool bit for bit -- plain, with the scenario, with kicks"""
    n = TP.N

    def build(entry, record, gait=False):
        ev = TP._evaluator(policy, n, **HZ)
        if mode == "scenario":
            TS._install(ev)
        elif mode == "kicks":
            TK._install(ev, False)
        if gait:
            ev.measure_gait()
        ev.entry_points = entry
        rec = _run(ev, [(TP.T1, persistent), (T - TP.T1, persistent)], record)
        return ev, rec
    old, r_old = build("auto", TP.ALL)
    null, r_null = build("measured", TP.ALL)
    only, r_only = build("auto", ALL)
    full, r_full = build("auto", ALL, gait=True)
    assert old.gait is None and null.gait is None and only.gait is None and full.gait is not None
    for ev, rec in ((null, r_null), (only, r_only), (full, r_full)):
        TP._assert_same_records(r_old, {k: v for k, v in rec.items() if k != "gait"})
        TS._same(old, ev, n)
    assert float(only.prev_contact.sum()) == 0 and float(full.prev_contact.sum()) > 0       # the recorder alone leaves prev_contact alone
    assert torch.equal(r_only["gait"], r_full["gait"]) and torch.equal(r_only["gait"][:, :, 0:12], r_old["torque"])
    assert float(full.gait[:, G["n"]].sum()) == T * n - float(r_old["done"].sum())


# ---- 5. refusals and capability ----
def test_the_persistent_form_is_refused_on_a_4_lane_pool(policy, monkeypatch):
    """a 4-lane pool: the persistent call is refused with the condition and the new entry point named, nothing has run; the five-launch form
    measures there"""
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", "4")
    ev = _install(TP._evaluator(policy, 6, **HZ), False)
    assert ev.env.lanes_per_robot == 4 and ev.persistent_supported is False
    with pytest.raises(RuntimeError, match="16-lane layout") as info:
        ev.run(3, persistent=True)
    assert "irrl_lstm_eval_measured_persistent" in str(info.value) and ev.t == 0 and float(ev.gait.sum()) == 0
    ev.run(T, persistent="auto")
    assert float(ev.gait[:, G["n"]].sum()) > 0 and ev.t == T


# ---- 6. the closed loop against the host-driven twin ----
MU, CMD, ROBOTS, WARM, STEPS = 0.8, 2.0, 8, 500, 500
BOUNDS = dict(power_mean=0.246, cot=1.41e-3, duty=3.2e-2, stride_hz=16.0)


def test_robustness_sweep_with_gait_agrees_with_the_host_driven_twin():
    """evaluate.robustness_sweep(gait=True) -- friction 0.8, command 2 m/s, delay 0, 8 robots, 500 warm-up + 500 measured steps, the persistent
    launch -- against evaluate.reference_rollout(gait=True) on the f64 oracle over the same window (evaluate.gait_from_record).
    The closed loop is chaotic in the last digits, so the bounds are TWICE the oracle's own f32-build-against-f64 difference of each quantity, measured
    on the CPU with this scenario (worst robot, worst leg) before any device run:
        mean power 0.123 W of 12.39 W (1.0e-2 relative) -> bound 0.246 W        CoT 7.03e-4 of 0.0701 -> 1.41e-3
        duty factor per leg 1.6e-2 of 0.41 .. 0.44 -> 3.2e-2                     touchdowns per second per leg 8 of 21 .. 32 -> 16
    The touchdown rate is NOT the gait generator's 1 / period = 5 Hz and is reported, not asserted: the contact flag is the last substep's, and a
    stance foot of this actor leaves the contact list for single substeps, so the control-rate flag chatters (21 .. 32 rising edges per second on the
    f64 oracle; the f32 build differs from it by up to 8).  Duty factor and power do not depend on the order of the flags and are tight.
    A duty factor is a count of stance frames over 500, so its bound is held in whole frames: the oracle's two builds differ by 8 frames, the bound is
    16 frames (0.032 as a quotient picks up an ulp either way).  Measured on the MI355X against the f64 twin: mean power 0.1175 W, CoT 6.73e-4, duty
    factor 16 frames (0.032: AT the bound, leg 1; the other legs 1 .. 7 frames), touchdowns per second 10."""
    cfg = load_env_cfg("bp5_manual_eval.yaml", num_envs=ROBOTS)
    rows = EV.robustness_sweep(ACTOR, cfg, [MU], [0], [CMD] * ROBOTS, warm_steps=WARM, steps=STEPS, persistent=True, gait=True)
    off = EV.robustness_sweep(ACTOR, cfg, [MU], [0], [CMD] * ROBOTS, warm_steps=WARM, steps=STEPS, persistent=True)
    assert len(rows) == ROBOTS and all({k: r[k] for k in o} == o for r, o in zip(rows, off)) and "cot" not in off[0]
    import oracle as O
    env = O.OracleVecEnv(cfg)
    rec = EV.reference_rollout(env, NumpyLstmActor.from_npz(ACTOR), cfg, np.zeros(ROBOTS, int), np.full(ROBOTS, CMD), WARM + STEPS, mu=np.full(ROBOTS, MU),
                               warm=WARM, gait=True)
    mass = env.get_state()[:, 154:167].sum(1)
    want = EV.gait_from_record(rec, WARM, WARM + STEPS, mass, cfg["control_dt"])
    assert int(rec["falls"].sum()) == 0 and all(r["falls"] == 0 and r["gait_frames"] == STEPS for r in rows)
    got = {k: np.array([r[k] for r in rows]) for k in want}
    worst = dict(power_mean=np.abs(got["power_mean"] - want["power_mean"]).max(), cot=np.abs(got["cot"] - want["cot"]).max(),
                 duty=max(np.abs(got["duty%d" % l] - want["duty%d" % l]).max() for l in range(4)),
                 stride_hz=max(np.abs(got["stride_hz%d" % l] - want["stride_hz%d" % l]).max() for l in range(4)))
    print()
    print("device | f64 twin: mean power %.4f | %.4f W, CoT %.5f | %.5f, duty %s | %s, touchdowns/s %s | %s (1 / period = 5 Hz is not what this counts)"
          % (got["power_mean"][0], want["power_mean"][0], got["cot"][0], want["cot"][0], [round(float(got["duty%d" % l][0]), 3) for l in range(4)],
             [round(float(want["duty%d" % l][0]), 3) for l in range(4)], [float(got["stride_hz%d" % l][0]) for l in range(4)],
             [float(want["stride_hz%d" % l][0]) for l in range(4)]))
    print("worst |device - twin|: " + ", ".join("%s %.3e (bound %.3e)" % (k, worst[k], BOUNDS[k]) for k in BOUNDS))
    for k in BOUNDS:
        if k == "duty":
            assert int(np.rint(worst[k] * STEPS)) <= int(np.rint(BOUNDS[k] * STEPS)) == 16, (k, worst[k], BOUNDS[k])
        else:
            assert worst[k] <= BOUNDS[k], (k, worst[k], BOUNDS[k])
