"""Device-resident evaluation of a trained policy: the reference's robustness study (run_bp_v5.py:300-470 -- friction, observation delay,
rate / action low-passes, command ramp) without a host round trip per control step.

  PolicyEvaluator     the evaluation loop on the GPU (C-ABI irrl_lstm_eval_rollout, kernels csrc/eval_rollout.hpp: five launches per control
                      step; irrl_lstm_eval_rollout_persistent, csrc/env_eval_kernels.hpp: the whole run as one persistent launch, bit-identical):
                      per-env delay and command, recorders, per-env f64 statistics.  The actor is a CustomLSTMPolicy or an MlpPolicy (64, 64)
                      (irrl_mlp_eval_measured[_persistent], csrc/env_eval_mlp_kernels.hpp: the same two forms)
  condition           numpy float64 twin of the loop's observation conditioning (command low-pass, delay line, rate low-pass, command overwrite)
  reference_rollout   numpy float64 twin of the whole loop around any env adapter with reset / step / get_state / set_contact_coeff: THE host-driven
                      evaluation loop (the test harnesses and tools translate their cases into one call of it)
  body_statistics     the statistics of a [frames, 13] body recording, of this build's loops and of the reference's simulator logs alike
  robustness_sweep    friction x delay x command grid in ONE Manual-mode pool -> one row of statistics per condition
  perturbation_study  the reference's perturbation exploration (Exp_Raw_Data/Param-*.txt): friction x delay conditions x explorations in ONE pool,
                      a warm-up, one random kick of every robot's base state, then the frames over which the ensemble converges or falls

Semantics of control step t (global counter, carried across `run` calls), per env:
   cmd = (1 - a_cmd) cmd + a_cmd cmd_target;  ring[t % D] = obs;  o = ring[(t - delay) mod D];
   o[17:29], o[32:35] = (1 - a_vel) vel_his + a_vel o;  vel_his = o;  o[0:3] = (cmd - mean) / std;
   a = actor(o) (deterministic, clipped; LSTM state reset where `done`);  a = (1 - a_act) act_his + a_act a;  act_his = a;
   env.step(a);  record;  cmd = 0 where done.
a = 2 pi dt f / (2 pi dt f + 1); f None or <= 0 means "filter off" (a = 1 exactly, the value passes unchanged).

A scenario (PolicyEvaluator.set_scenario; the keywords of condition / reference_rollout; robustness_sweep's levels / heading), with
tau = max(t - t0, 0): cmd_target of step t is row min(tau // cmd_every, S - 1) of a command table (staircase_schedule: the script's `--step`);
the heading hold (heading_hold: the script's `--dir_fd`) replaces o[2] by the scaled output of a PI loop on the base yaw in front of the step,
err = wrap(ref - yaw), I = clip(I + err dt, -W, W), out = kp err + ki I, I = 0 where done; the frame of step t goes to statistics bucket
min(tau // stat_every, B - 1).

A kick table (set_scenario's / reference_rollout's kicks, kick_first, kick_every; kick_rows, apply_kick, exploration_kicks, perturbation_study):
row r of kicks [R, N, 11] displaces the robots' base state at the start of env step t = t0 + kick_first + r kick_every -- behind the actor and the
action filter of step t, on the state step t - 1 left; see kick_rows for the row and apply_kick for the arithmetic.

Gait measurements (set_scenario's gait / measure_gait, run's "gait" recorder; gait_rows_numpy, gait_from_sums, reference_rollout's gait): behind
every env step that does not end in `done`, the joint mechanical power sum_j tq_j qd_j, torque sums, contact flags and ground impulses of the pool
are added to f64 sums [B, 20, N] in the statistics' buckets (Figure2.py:62-63, :198-222 of the reference: power and cost of transport per command
level); see gait_from_sums for what comes out.

Analyses of the gait recorder (footfall_numpy / footfall_device / footfall_row, motor_plane_numpy / motor_plane_device / motor_plane_row,
robustness_sweep's footfall / motor): the reference's debounced contact flags (Figure2.py:97-116) with stride, stance, swing and leg-phase
statistics, and its motor torque-speed plane (Figure5.py) per condition and joint, on the device; include/irrl_env.h has the rules.
"""
import ctypes as C
import math

import numpy as np

from .helper import obs_normalisation

# offsets into the flat per-env state of get_state() (include/irrl_env.h IRRL_S_*)
_S_GC, _S_GV, _S_TORQUE = 0, 19, 61
# rows of the device statistics (include/irrl_env.h IRRL_EVAL_STAT_*)
STAT_SLOTS = ("n", "vx", "vx2", "z", "z2", "roll", "roll2", "pitch", "pitch2", "wx", "wx2", "wy", "wy2", "vz", "vz2", "vy", "wz", "falls")
WORK_DIM = 80            # IRRL_EVAL_WORK_DIM
# what robustness_sweep and `run_bp_v5.py --test --sweep` do unless told otherwise (PolicyEvaluator.run's own default stays False): the persistent
# launch where it exists -- measured faster at both pool sizes, 36.5 against 58.5 us per control step at 4096 envs and 36.0 against 55.1 us at 90
# 
PERSISTENT_DEFAULT = "auto"


def mlp_auto_persistent(n):
    """does persistent="auto" take the persistent launch for an MlpPolicy on a pool of n robots?  Only at the pool sizes where its median time per
    control step measured below the per-step form's: it did at both sizes measured, 30.1 against 49.0 us at 4096 robots and 30.2 against 45.7 us
    at 90 (MI355X, profiles/eval_mlp_mi355x.log), so every size takes it."""
    return True
RECORDERS = {"obs_cond": 35, "act_clipped": 12, "act_applied": 12, "body": 13, "torque": 12, "obs_raw": 35, "reward": 0, "done": 0}   # C argument order


def lowpass_alpha(dt, hz):
    """coefficient of the script's first-order low-pass (run_bp_v5.py:83); None / <= 0: the filter is off (exactly 1.0)"""
    if hz is None or not hz > 0:
        return 1.0
    w = 2.0 * math.pi * float(dt) * float(hz)
    return w / (w + 1.0)


def contact_material(mu):
    """friction coefficient(s) mu [n] -> the [n, 3] float32 rows of SetContactCoefficient: (mu, restitution 0.2, restitution threshold 0.01), the
    material of the evaluation script (run_bp_v5.py:317)"""
    mu = np.atleast_1d(np.asarray(mu, np.float32))
    return np.stack([mu, np.full_like(mu, 0.2), np.full_like(mu, 0.01)], 1)


def _cmd_rows(cmd, n):
    """[n] forward-velocity commands or [n, 3] (vx, vy, omega) -> [n, 3] float64"""
    c = np.asarray(cmd, np.float64)
    if c.ndim == 0:
        c = np.full(n, float(c))
    if c.ndim == 1:
        c = np.stack([c, np.zeros_like(c), np.zeros_like(c)], 1)
    if c.shape != (n, 3):
        raise ValueError("cmd must have shape (%d,) or (%d, 3)" % (n, n))
    return c


def _step_rows(v, n, what):
    """a scalar or [n] whole numbers of control steps -> [n] int64"""
    v = np.asarray(v)
    if v.ndim == 0:
        v = np.full(n, int(v))
    if v.shape != (n,) or np.any(v != np.floor(v)):
        raise ValueError("%s must be %d whole numbers of control steps" % (what, n))
    return v.astype(np.int64)


def _delay_rows(delay, n, depth=None):
    d = _step_rows(delay, n, "delay")
    depth = int(d.max()) + 1 if depth is None else int(depth)
    if depth < 1 or d.min() < 0 or d.max() >= depth:
        raise ValueError("0 <= delay < depth (%d) violated: delays span %d .. %d" % (depth, d.min(), d.max()))
    return d, depth


# ---- the scenario: command schedule, heading hold (run_bp_v5.py:383-388 `--step`, :308-315 / :400-406 `--dir_fd`) ----
def _schedule_rows(cmd_schedule, n):
    """[S, n] forward-velocity commands or [S, n, 3] -> [S, n, 3] float64"""
    c = np.asarray(cmd_schedule, np.float64)
    if c.ndim == 2:
        c = np.stack([c, np.zeros_like(c), np.zeros_like(c)], 2)
    if c.ndim != 3 or c.shape[0] < 1 or c.shape[1:] != (n, 3):
        raise ValueError("cmd_schedule must have shape (S, %d) or (S, %d, 3) with S >= 1" % (n, n))
    return c


def staircase_schedule(cmds, levels=4):
    """the script's command staircase (run_bp_v5.py:383-388: `(t // 5000 + 1) / 4 * cmd`): cmds [n] or [n, 3] -> [levels, n, 3], row l =
    (l + 1) / levels * cmd; held `cmd_every` control steps per row by the caller"""
    levels = int(levels)
    if levels < 1:
        raise ValueError("levels >= 1")
    c = np.asarray(cmds, np.float64)
    c = _cmd_rows(c, c.shape[0] if c.ndim else 1)
    return np.stack([(l + 1) / levels * c for l in range(levels)], 0)


def yaw_from_quaternion(q):
    """q [..., 4] = w x y z -> yaw (utils/Rotation.py:8): atan2(2 (w z + x y), 1 - 2 (y^2 + z^2))"""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def wrap_angle(a):
    """into [-pi, pi)"""
    a = np.asarray(a, np.float64)
    return a - 2 * np.pi * np.floor((a + np.pi) / (2 * np.pi))


def heading_hold(n, ref=0.0, kp=1.0, ki=0.1, windup=None):
    """the heading hold of `n` envs: ref / kp / ki a scalar or [n] each (the reference's gains, run_bp_v5.py:311-313), windup the integrator's
    clamp (None: the config's Omega).  An env with kp == ki == 0 runs without it."""
    return dict(ref=np.broadcast_to(np.asarray(ref, np.float64), (n,)).copy(), kp=np.broadcast_to(np.asarray(kp, np.float64), (n,)).copy(),
                ki=np.broadcast_to(np.asarray(ki, np.float64), (n,)).copy(), windup=windup)


def heading_parameters(heading, n, omega, dt):
    """a `heading` dict (ref, kp, ki scalars or [n]; windup, dt optional) -> the same with [n] float64 arrays, windup and dt filled in"""
    if heading is None:
        return None
    h = heading_hold(n, heading.get("ref", 0.0), heading.get("kp", 1.0), heading.get("ki", 0.1), heading.get("windup"))
    h["windup"] = float(omega if h["windup"] is None else h["windup"])
    h["dt"] = float(heading.get("dt") or dt)
    if h["windup"] < 0 or not h["dt"] > 0:
        raise ValueError("heading: windup >= 0 and dt > 0")
    return h


def schedule_row(t, t0, every, rows):
    """min(max(t - t0, 0) // every, rows - 1): the row of a command table / the statistics bucket of control step t"""
    return min(max(int(t) - int(t0), 0) // int(every), int(rows) - 1)


# ---- the kick table: base-state displacements at chosen control steps (include/irrl_env.h irrl_eval_kicks; csrc/eval_elements.hpp) ----
KICK_DIM = 11            # IRRL_EVAL_KICK_DIM: dz | dq w x y z | dv x y z | dw x y z
# the perturbation amplitudes of the reference's Exp_Raw_Data/Param-*.txt, in the files' order
NOISE_KEYS = ("z_noise", "roll_noise", "pitch_noise", "x_dot_noise", "y_dot_noise", "z_dot_noise", "roll_dot_noise", "pitch_dot_noise", "yaw_dot_noise")


def quaternion_product(a, b):
    """a (x) b for quaternions [..., 4] = w x y z (Hamilton), float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def rotation_matrix(q):
    """q [..., 4] = w x y z (unit) -> R [..., 3, 3], body -> world"""
    q = np.asarray(q, np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def kick_rows(dz=0.0, roll=0.0, pitch=0.0, yaw=0.0, dv=(0.0, 0.0, 0.0), dw=(0.0, 0.0, 0.0)):
    """Kick rows [..., 11] float32 = dz | dq_w dq_x dq_y dq_z | dv_x dv_y dv_z | dw_x dw_y dw_z from increments that broadcast against each other
    (dz, roll, pitch, yaw: [...]; dv, dw: [..., 3]).  Everything is BODY-FRAME: with q the base quaternion and R(q) its rotation matrix before
    the kick, z += dz, v_world += R(q) dv, w_world += R(q) dw, q = normalised(q (x) dq).  Convention of dq, computed here in float64 (the device
    does no trigonometry): dq = q_z(yaw) (x) q_y(pitch) (x) q_x(roll) with q_x(a) = (cos a/2, sin a/2, 0, 0) etc. -- intrinsic z-y'-x'', i.e. the
    roll / pitch / yaw of body_frame() applied to an upright base give back these three angles.  All angles zero is the IDENTITY kick
    dq = (1, 0, 0, 0), a real kick (it renormalises q).  "No kick for this env" is a row whose four dq words are zero: np.zeros(11)."""
    dz, roll, pitch, yaw = (np.asarray(v, np.float64) for v in (dz, roll, pitch, yaw))
    dv, dw = np.asarray(dv, np.float64), np.asarray(dw, np.float64)
    if dv.shape[-1:] != (3,) or dw.shape[-1:] != (3,):
        raise ValueError("dv and dw end in an axis of 3")
    shape = np.broadcast_shapes(dz.shape, roll.shape, pitch.shape, yaw.shape, dv.shape[:-1], dw.shape[:-1])
    half = lambda a: np.broadcast_to(a, shape) / 2.0
    zero = np.zeros(shape)
    qx = np.stack([np.cos(half(roll)), np.sin(half(roll)), zero, zero], -1)
    qy = np.stack([np.cos(half(pitch)), zero, np.sin(half(pitch)), zero], -1)
    qz = np.stack([np.cos(half(yaw)), zero, zero, np.sin(half(yaw))], -1)
    out = np.zeros(shape + (KICK_DIM,))
    out[..., 0] = np.broadcast_to(dz, shape)
    out[..., 1:5] = quaternion_product(quaternion_product(qz, qy), qx)
    out[..., 5:8] = np.broadcast_to(dv, shape + (3,))
    out[..., 8:11] = np.broadcast_to(dw, shape + (3,))
    return out.astype(np.float32)


def kick_on(rows):
    """which kick rows [..., 11] displace their env: the ones with a non-zero dq word"""
    return np.any(np.asarray(rows)[..., 1:5] != 0, -1)


def apply_kick(state_rows, rows):
    """The float64 twin of the device's kick (csrc/eval_elements.hpp irrl_eval_kick_apply): state_rows [n, 288] (get_state), rows [n, 11] -> a new
    [n, 288] with gc[2], gc[3:7], gv[0:3], gv[3:6] of the envs whose row is on (kick_on) displaced; everything else, and every env whose row is off,
    is a copy."""
    s = np.array(state_rows, np.float64)
    k = np.asarray(rows, np.float64)
    if s.ndim != 2 or k.shape != (s.shape[0], KICK_DIM):
        raise ValueError("apply_kick: state rows [n, 288] and kick rows [n, %d]" % KICK_DIM)
    on = kick_on(k)
    q = s[:, _S_GC + 3:_S_GC + 7]
    R = rotation_matrix(q)
    z = s[:, _S_GC + 2] + k[:, 0]
    v = s[:, _S_GV:_S_GV + 3] + np.einsum("nij,nj->ni", R, k[:, 5:8])
    w = s[:, _S_GV + 3:_S_GV + 6] + np.einsum("nij,nj->ni", R, k[:, 8:11])
    qn = quaternion_product(q, k[:, 1:5])
    norm = np.sqrt((qn * qn).sum(-1, keepdims=True))
    qn = qn / np.where(norm > 0, norm, 1.0)
    s[on, _S_GC + 2] = z[on]
    s[on, _S_GC + 3:_S_GC + 7] = qn[on]
    s[on, _S_GV:_S_GV + 3] = v[on]
    s[on, _S_GV + 3:_S_GV + 6] = w[on]
    return s


def kick_row_index(t, t0, kick_first, kick_every, rows):
    """the row of a kick table that fires at control step t, or -1: t >= t0 + kick_first and t - t0 - kick_first = r kick_every, 0 <= r < rows.
    In t, not in tau = max(t - t0, 0): nothing fires in front of t0 + kick_first."""
    d = int(t) - int(t0) - int(kick_first)
    if d < 0 or d % int(kick_every) != 0 or d // int(kick_every) >= int(rows):
        return -1
    return d // int(kick_every)


def _kick_table(kicks, n):
    """[n, 11] or [R, n, 11] -> [R, n, 11] float32"""
    k = np.asarray(kicks, np.float32)
    if k.ndim == 2:
        k = k[None]
    if k.ndim != 3 or k.shape[0] < 1 or k.shape[1:] != (n, KICK_DIM):
        raise ValueError("kicks must have shape (%d, %d) or (R, %d, %d) with R >= 1" % (n, KICK_DIM, n, KICK_DIM))
    return np.ascontiguousarray(k)


def _kick_schedule(kick_first, kick_every):
    kick_first, kick_every = int(kick_first), int(kick_every)
    if kick_first < 0 or kick_every < 1:
        raise ValueError("kick_first >= 0 and kick_every >= 1")
    return kick_first, kick_every


def exploration_kicks(n, noise, rng):
    """`n` random kick rows [n, 11] float32 of the reference's perturbation exploration: every component uniform in [-a, a] with a = noise[key] for
    the keys of the Exp_Raw_Data/Param-*.txt files (NOISE_KEYS; a missing key is 0): z_noise -> dz, roll_noise / pitch_noise -> the attitude
    increment (yaw is not perturbed), x_dot_noise / y_dot_noise / z_dot_noise -> dv, roll_dot_noise / pitch_dot_noise / yaw_dot_noise -> dw, all
    body-frame (kick_rows).  rng: a numpy Generator; the nine components are drawn in the order of NOISE_KEYS, n values each, zero amplitudes
    included, so a draw does not depend on which amplitudes are set.
    The reference's exploration harness is not in its tree -- only the amplitudes are on record -- so the uniform distribution and the body frame
    are THIS build's choice."""
    unknown = sorted(set(noise) - set(NOISE_KEYS))
    if unknown:
        raise KeyError("unknown noise key(s) %s: choose from %s" % (unknown, list(NOISE_KEYS)))
    n = int(n)
    d = {}
    for k in NOISE_KEYS:
        a = float(noise.get(k, 0.0))
        if a < 0:
            raise ValueError("%s >= 0" % k)
        d[k] = rng.uniform(-1.0, 1.0, n) * a
    return kick_rows(dz=d["z_noise"], roll=d["roll_noise"], pitch=d["pitch_noise"], dv=np.stack([d["x_dot_noise"], d["y_dot_noise"], d["z_dot_noise"]], 1),
                     dw=np.stack([d["roll_dot_noise"], d["pitch_dot_noise"], d["yaw_dot_noise"]], 1))


def perturb_base(env_impl, rows):
    """displace the robots of an initialised FlexibleGymEnv NOW, one kick row per env (kick_rows): rows a torch tensor [N, 11] float32 on the
    pool's device (stream-ordered on the pool's stream, no synchronisation) or anything numpy takes (copied over; waits for the stream)"""
    from . import _lib
    from ._lib import ptr
    n = env_impl.getNumOfEnvs()
    lib = _lib.load()
    if hasattr(rows, "is_cuda"):
        import torch
        if not rows.is_cuda or rows.dtype != torch.float32 or tuple(rows.shape) != (n, KICK_DIM) or not rows.is_contiguous():
            raise TypeError("rows: a contiguous float32 tensor [%d, %d] on the pool's device" % (n, KICK_DIM))
        _lib.check(lib.irrl_env_perturb_base(env_impl._h, ptr(rows)))
    else:
        k = np.ascontiguousarray(rows, np.float32)
        if k.shape != (n, KICK_DIM):
            raise TypeError("rows must have shape (%d, %d)" % (n, KICK_DIM))
        _lib.check(lib.irrl_env_perturb_base_host(env_impl._h, k.ctypes.data_as(C.POINTER(C.c_float))))


# ---- the gait measurements: joint power, cost of transport, footfall pattern (include/irrl_env.h irrl_eval_gait; csrc/eval_elements.hpp) ----
# rows of the device sums (IRRL_EVAL_GAIT_*); the three peak_* rows are running maxima, every other row is a sum
GAIT_SLOTS = ("n", "p", "p2", "ppos", "pneg", "tau2", "tau2_knee", "peak_tau", "peak_qd", "stance0", "stance1", "stance2", "stance3",
              "touchdown0", "touchdown1", "touchdown2", "touchdown3", "flight", "grfz", "peak_grf")
GAIT_PEAKS = tuple(GAIT_SLOTS.index(k) for k in ("peak_tau", "peak_qd", "peak_grf"))
GAIT_REC_DIM = 32        # IRRL_EVAL_GAIT_REC_DIM: tq 12 | qd 12 | in_contact 4 | lam_w_z / control_dt 4
_S_LAMW, _S_INCONTACT, _S_MASS = 135, 147, 154
COT_VX_FLOOR = 0.05      # m/s: below this |mean v_x| a cost of transport is a division by noise, reported as NaN


def gait_rows_numpy(rec_gait, rec_done, stat_buckets=1, stat_every=1, t=0, t0=0, prev_contact=None, sums=None, lamw=None, inv_control_dt=None):
    """The float64 twin of the device's gait epilogue (csrc/eval_elements.hpp irrl_eval_gait_epilogue): rec_gait [T, N, 32] and rec_done [T, N] of
    control steps t .. t + T - 1 -> (sums [stat_buckets, 20, N] float64 in the rows of GAIT_SLOTS, prev_contact [N, 4] uint8), with the bucket rule
    of schedule_row(t, t0, stat_every, stat_buckets).  Sequential float64 adds in the device's order -- joints 0 .. 11, legs 0 .. 3, steps in
    turn -- so the rows whose arithmetic is exact are the device's bit for bit.  prev_contact / sums: the state a previous call left (default: a
    fresh evaluation, zeros).  The recorder holds only the z component of the impulse, so the peak_grf row needs lamw [T, N, 4, 3] (the pool's
    lam_w) and inv_control_dt (float32); without them that row is NaN."""
    rec = np.asarray(rec_gait)
    done = np.asarray(rec_done).astype(bool)
    T, N = done.shape
    if rec.shape != (T, N, GAIT_REC_DIM):
        raise ValueError("rec_gait [T, N, %d] and rec_done [T, N]" % GAIT_REC_DIM)
    B = max(int(stat_buckets), 1)
    G = {k: i for i, k in enumerate(GAIT_SLOTS)}
    out = np.zeros((B, len(GAIT_SLOTS), N)) if sums is None else np.array(sums, np.float64).reshape(B, len(GAIT_SLOTS), N)
    prev = np.zeros((N, 4), np.uint8) if prev_contact is None else np.array(prev_contact, np.uint8).reshape(N, 4)
    tq, qd, fz = rec[:, :, 0:12].astype(np.float64), rec[:, :, 12:24].astype(np.float64), rec[:, :, 28:32].astype(np.float64)
    contact = rec[:, :, 24:28] != 0
    for k in range(T):
        g = out[schedule_row(t + k, t0, stat_every, B)]
        live = ~done[k]
        p, ppos, pneg, tau2, tau2k, ptau, pqd = (np.zeros(N) for _ in range(7))
        for j in range(12):
            tw = tq[k, :, j] * qd[k, :, j]
            p = p + tw
            ppos = ppos + np.where(tw > 0, tw, 0.0)
            pneg = pneg + np.where(tw < 0, tw, 0.0)
            tt = tq[k, :, j] * tq[k, :, j]
            if j % 3 == 2:
                tau2k = tau2k + tt
            else:
                tau2 = tau2 + tt
            ptau, pqd = np.maximum(ptau, np.abs(tq[k, :, j])), np.maximum(pqd, np.abs(qd[k, :, j]))
        grfz, pgrf = np.zeros(N), np.zeros(N)
        for l in range(4):
            c = contact[k, :, l]
            g[G["stance0"] + l] += np.where(live & c, 1.0, 0.0)
            g[G["touchdown0"] + l] += np.where(live & c & (prev[:, l] == 0), 1.0, 0.0)
            grfz = grfz + np.where(c, fz[k, :, l], 0.0)
            if lamw is not None:
                v = np.asarray(lamw)[k, :, l].astype(np.float64)
                f = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]) * np.float64(np.float32(inv_control_dt))
                pgrf = np.maximum(pgrf, np.where(c, f, 0.0))
        add = lambda key, v: g.__setitem__(G[key], g[G[key]] + np.where(live, v, 0.0))
        peak = lambda key, v: g.__setitem__(G[key], np.maximum(g[G[key]], np.where(live, v, 0.0)))
        add("n", 1.0); add("p", p); add("p2", p * p); add("ppos", ppos); add("pneg", pneg); add("tau2", tau2); add("tau2_knee", tau2k)
        peak("peak_tau", ptau); peak("peak_qd", pqd)
        add("flight", np.where(contact[k].any(1), 0.0, 1.0)); add("grfz", grfz); peak("peak_grf", pgrf)
        prev = contact[k].astype(np.uint8)
    if lamw is None:
        out[:, G["peak_grf"]] = np.nan
    return out, prev


def gait_merge(sums):
    """gait sums [B, 20, n] of several buckets -> [20, n] of the whole window: the sum rows added, the peak rows maximised"""
    s = np.asarray(sums, np.float64)
    if s.ndim == 2:
        return s
    out = s.sum(0)
    for i in GAIT_PEAKS:
        out[i] = s[:, i].max(0)
    return out


def gait_from_sums(sums, stats_sums, mass, control_dt, g=9.81, vx_floor=COT_VX_FLOOR):
    """gait sums [20, n] (GAIT_SLOTS) and the body statistics' sums [18, n] (STAT_SLOTS) of the same window -> dict of [n] arrays:
    power_mean, power_std (W, p = sum_j tq_j qd_j per control step: Figure2.py:62-63), power_pos, power_neg (mean positive / negative joint work
    rate), cot = power_mean / (mass g mean v_x) (Figure2.py:198-222; NaN where |mean v_x| < vx_floor m/s or no frame was added), duty0 .. duty3
    (stance frames / frames), stride_hz0 .. stride_hz3 (touchdowns of the RAW contact flag / window seconds, the window being frames * control_dt:
    a raw touchdown rate, several times the stride frequency, because the control-rate flag chatters while a foot is down -- the debounced stride
    frequency is footfall_row's stride_hz<l>, out of irrl_eval_footfall), flight (fraction of
    frames with no leg in contact), grfz_bw (mean of sum_legs lam_w_z / control_dt over mass g; see include/irrl_env.h for the unit), tau2_mean,
    tau2_knee_mean (joint side; the knee motor sits behind a 1.55 reduction, Figure2.py:32-34), peak_tau, peak_qd, peak_grf, gait_frames.
    mass: [n] or a scalar (the reference's figure uses m = 10, g = 9.8)."""
    s = {k: np.asarray(sums[i], np.float64) for i, k in enumerate(GAIT_SLOTS)}
    b = {k: np.asarray(stats_sums[i], np.float64) for i, k in enumerate(STAT_SLOTS)}
    some = s["n"] > 0
    cnt = np.maximum(s["n"], 1.0)
    mass = np.broadcast_to(np.asarray(mass, np.float64), s["n"].shape)
    weight = mass * float(g)
    pm = s["p"] / cnt
    vx = b["vx"] / np.maximum(b["n"], 1.0)
    ok = some & (np.abs(vx) >= float(vx_floor))
    out = {"power_mean": pm, "power_std": np.sqrt(np.maximum(s["p2"] / cnt - pm * pm, 0.0)), "power_pos": s["ppos"] / cnt, "power_neg": s["pneg"] / cnt,
           "cot": np.where(ok, pm / (weight * np.where(ok, vx, 1.0)), np.nan)}
    seconds = cnt * float(control_dt)
    for l in range(4):
        out["duty%d" % l] = s["stance%d" % l] / cnt
        out["stride_hz%d" % l] = s["touchdown%d" % l] / seconds
    out.update({"flight": s["flight"] / cnt, "grfz_bw": s["grfz"] / cnt / weight, "tau2_mean": s["tau2"] / cnt, "tau2_knee_mean": s["tau2_knee"] / cnt,
                "peak_tau": s["peak_tau"], "peak_qd": s["peak_qd"], "peak_grf": s["peak_grf"], "gait_frames": s["n"].astype(np.int64)})
    return out


def gait_from_record(rec, lo, hi, mass, control_dt, g=9.81, vx_floor=COT_VX_FLOOR):
    """gait_from_sums over the control steps lo .. hi - 1 of a reference_rollout(..., gait=True) record: the twin's sums of rec["gait"] / rec["done"]
    (the contact flags of step lo - 1 as prev_contact) and the mean body-frame v_x of rec["body"] over the same steps"""
    lo, hi = int(lo), int(hi)
    prev = (np.asarray(rec["gait"])[lo - 1, :, 24:28] != 0).astype(np.uint8) if lo > 0 else None
    sums, _ = gait_rows_numpy(rec["gait"][lo:hi], rec["done"][lo:hi], prev_contact=prev)
    n = sums.shape[2]
    body = np.zeros((len(STAT_SLOTS), n))
    body[STAT_SLOTS.index("n")] = hi - lo
    body[STAT_SLOTS.index("vx")] = [body_frame(np.asarray(rec["body"])[lo:hi, e])[0][:, 0].sum() for e in range(n)]
    return gait_from_sums(sums[0], body, mass, control_dt, g, vx_floor)


def gait_record_from_state(state_rows, control_dt):
    """the recorder's 32 words [n, 32] float64 out of get_state() rows [n, 288]: torque | gv[6:18] | in_contact | lam_w_z / control_dt"""
    s = np.asarray(state_rows, np.float64)
    return np.concatenate([s[:, _S_TORQUE:_S_TORQUE + 12], s[:, _S_GV + 6:_S_GV + 18], (s[:, _S_INCONTACT:_S_INCONTACT + 4] != 0).astype(np.float64),
                           s[:, _S_LAMW + 2:_S_LAMW + 12:3] / float(control_dt)], 1)


# ---- numpy float64 twin ----
def condition_state(ob0, depth):
    """state of `condition` after a reset: the reset observation fills the whole delay line, command, history and heading integrator are zero"""
    ob0 = np.asarray(ob0, np.float64)
    return dict(ring=np.repeat(ob0[None], int(depth), 0), cmd=np.zeros((ob0.shape[0], 3)), vel_his=np.zeros_like(ob0), heading_int=np.zeros(ob0.shape[0]),
                heading_out=np.zeros(ob0.shape[0]))


def condition(state, t, obs, delay, cmd_target, a_cmd, a_vel, mean3, std3, *, cmd_schedule=None, cmd_every=1, heading=None, t0=0, yaw=None):
    """steps 1-6 of control step `t` for a batch: obs [n, 35] raw observation -> what the actor sees.  Updates `state` in place.
    cmd_schedule [S, n, 3] / cmd_every / t0: the target is the schedule's row schedule_row(t, t0, cmd_every, S) in place of cmd_target.
    heading (a dict of [n] ref, kp, ki and windup, dt) with yaw [n], the base yaw in front of the step: element 2 of the envs with a non-zero gain
    is the scaled PI output, state["heading_int"] the integrator, state["heading_out"] the output (0 where off)."""
    ring = state["ring"]
    depth = ring.shape[0]
    rows = np.arange(ring.shape[1])
    if cmd_schedule is not None:
        cmd_target = np.asarray(cmd_schedule, np.float64)[schedule_row(t, t0, cmd_every, len(cmd_schedule))]
    state["cmd"] = (1 - a_cmd) * state["cmd"] + a_cmd * cmd_target if a_cmd != 1.0 else np.array(cmd_target, np.float64)
    ring[t % depth] = np.asarray(obs, np.float64)
    o = ring[(t - np.asarray(delay)) % depth, rows].copy()
    if a_vel != 1.0:
        o[:, 32:35] = (1 - a_vel) * state["vel_his"][:, 32:35] + a_vel * o[:, 32:35]
        o[:, 17:29] = (1 - a_vel) * state["vel_his"][:, 17:29] + a_vel * o[:, 17:29]
    state["vel_his"] = o.copy()
    o[:, 0:3] = (state["cmd"] - mean3) / std3
    if heading is not None:
        on = (heading["kp"] != 0) | (heading["ki"] != 0)
        err = wrap_angle(heading["ref"] - np.asarray(yaw, np.float64))
        integ = np.clip(state["heading_int"] + err * heading["dt"], -heading["windup"], heading["windup"])
        out = heading["kp"] * err + heading["ki"] * integ
        state["heading_int"] = np.where(on, integ, state["heading_int"])
        state["heading_out"] = np.where(on, out, 0.0)
        o[on, 2] = (out[on] - mean3[2]) / std3[2]
    return o


def reference_rollout(env, actor, env_cfg, delay, cmd, steps, cmd_hz=1.0, vel_hz=None, act_hz=None, mu=None, warm=0, mu_warm=0.8, depth=None, *,
                      cmd_schedule=None, cmd_every=1, heading=None, t0=0, kicks=None, kick_first=0, kick_every=1, gait=False):
    """The evaluation loop in numpy float64 around `env` (reset() -> ob, step(a) -> ob, reward, done, extra, get_state() -> [n, 288],
    set_contact_coeff([n, 3])) and `actor` (act(o [n, 35], done [n]) -> [n, 12], already clipped if it clips).
    mu [n]: friction per env (contact_material); env i runs on mu_warm until step warm[i] (a scalar or [n]) and on mu[i] from then on, warm[i] = 0:
    from the start.  set_contact_coeff is called before the reset and at the steps where some env switches.  None leaves the env's material alone.
    The actor's float64 action goes through the action low-pass as it is and becomes float32 once, at env.step.
    -> dict of per-step records body [steps, n, 13], torque, obs_raw, obs_cond, act_clipped, act_applied, reward, done, and falls [n]; a window
    warm[i] : warm[i] + frames is the caller's slice.
    cmd_schedule [S, n] or [S, n, 3] with cmd_every and t0: the command schedule of PolicyEvaluator.set_scenario in place of `cmd`; heading: a
    heading_hold dict -- the yaw comes from env.get_state() in front of the step, in float64; the record gains heading_out [steps, n] (the PI
    output, 0 where the hold is off).
    kicks [n, 11] or [R, n, 11] with kick_first, kick_every (and t0): row kick_row_index(t, ...) displaces the base state through apply_kick and
    env.get_state() / env.set_state() behind the action filter of step t, in front of env.step.
    gait: the record gains gait [steps, n, 32], the words of the device's rec_gait out of env.get_state() behind every step (gait_record_from_state;
    feed it to gait_rows_numpy with the record's done)."""
    n = env.n
    delay, depth = _delay_rows(delay, n, depth)
    target = _cmd_rows(cmd, n)
    mean, std, _, _ = obs_normalisation(env_cfg)
    dt = float(env_cfg["control_dt"])
    schedule = None if cmd_schedule is None else _schedule_rows(cmd_schedule, n)
    heading = heading_parameters(heading, n, float(env_cfg["Omega"]) if heading is not None else 0.0, dt)
    a_cmd, a_vel, a_act = lowpass_alpha(dt, cmd_hz), lowpass_alpha(dt, vel_hz), lowpass_alpha(dt, act_hz)
    warm = _step_rows(warm, n, "warm")
    if kicks is not None:
        kicks = _kick_table(kicks, n)
        kick_first, kick_every = _kick_schedule(kick_first, kick_every)
    if mu is not None:
        mu = np.broadcast_to(np.asarray(mu, np.float64), (n,))
        coeff = contact_material(np.where(warm == 0, mu, mu_warm))
        env.set_contact_coeff(coeff)
    ob = env.reset()
    st = condition_state(ob, depth)
    act_his = np.zeros((n, 12))
    done = np.zeros(n, bool)
    rec = dict(body=np.zeros((steps, n, 13)), torque=np.zeros((steps, n, 12)), obs_raw=np.zeros((steps, n, 35)), obs_cond=np.zeros((steps, n, 35)),
               act_clipped=np.zeros((steps, n, 12)), act_applied=np.zeros((steps, n, 12)), reward=np.zeros((steps, n)), done=np.zeros((steps, n), bool),
               heading_out=np.zeros((steps, n)))
    if gait:
        rec["gait"] = np.zeros((steps, n, GAIT_REC_DIM))
    for t in range(steps):
        switch = (warm == t) & (warm > 0)
        if mu is not None and switch.any():
            coeff[switch, 0] = mu[switch]
            env.set_contact_coeff(coeff)
        yaw = yaw_from_quaternion(np.asarray(env.get_state(), np.float64)[:, _S_GC + 3:_S_GC + 7]) if heading is not None else None
        o = condition(st, t, ob, delay, target, a_cmd, a_vel, mean[0:3], std[0:3], cmd_schedule=schedule, cmd_every=cmd_every, heading=heading, t0=t0, yaw=yaw)
        rec["heading_out"][t] = st["heading_out"]
        a = actor.act(o, done)
        rec["obs_cond"][t] = o
        rec["act_clipped"][t] = a
        if a_act != 1.0:
            a = (1 - a_act) * act_his + a_act * a
        act_his = np.asarray(a, np.float64)
        rec["act_applied"][t] = a
        r = kick_row_index(t, t0, kick_first, kick_every, len(kicks)) if kicks is not None else -1
        if r >= 0:
            env.set_state(apply_kick(env.get_state(), kicks[r]))
        ob, rew, done, _ = env.step(np.asarray(a, np.float32))
        s = env.get_state()
        rec["body"][t, :, 0:7] = s[:, _S_GC:_S_GC + 7]
        rec["body"][t, :, 7:13] = s[:, _S_GV:_S_GV + 6]
        rec["torque"][t] = s[:, _S_TORQUE:_S_TORQUE + 12]
        if gait:
            rec["gait"][t] = gait_record_from_state(s, dt)
        rec["obs_raw"][t] = ob
        rec["reward"][t] = rew
        rec["done"][t] = done
        st["cmd"][np.asarray(done, bool)] = 0.0              # the env restarted from rest
        st["heading_int"][np.asarray(done, bool)] = 0.0
    rec["falls"] = rec["done"].sum(0).astype(int)
    return rec


def body_frame(frames):
    """frames [n, 13] = base x y z, quaternion wxyz, world linear velocity, world angular velocity -> (linear velocity [n, 3] and angular velocity
    [n, 3] in the body frame, roll [n], pitch [n])"""
    d = np.asarray(frames, np.float64)
    w, x, y, z = d[:, 3], d[:, 4], d[:, 5], d[:, 6]
    R = np.zeros((len(d), 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (w * y + x * z)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (w * x + y * z); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    vb = np.einsum("nji,nj->ni", R, d[:, 7:10])
    wb = np.einsum("nji,nj->ni", R, d[:, 10:13])
    roll = np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
    pitch = np.arcsin(np.clip(2 * (w * y - x * z), -1, 1))
    return vb, wb, roll, pitch


def body_statistics(frames, window=None):
    """frames [n, 13] (layout of body_frame, 500 Hz) -> the statistics tests/golden/raisim_body_logs.json holds for each RaiSim log, taken over
    `window` (a slice; default: every frame), plus the whole series `vx_body` [n]"""
    d = np.asarray(frames, np.float64)
    h = window if window is not None else slice(0, len(d))
    vb, wb, roll, pitch = body_frame(d)
    return {"vx_body_mean": float(vb[h, 0].mean()), "vx_body_std": float(vb[h, 0].std()), "vy_body_mean": float(vb[h, 1].mean()),
            "z_mean": float(d[h, 2].mean()), "z_std": float(d[h, 2].std()), "roll_std": float(roll[h].std()),
            "pitch_mean": float(pitch[h].mean()), "pitch_std": float(pitch[h].std()), "yaw_rate_mean": float(d[h, 12].mean()),
            "roll_rate_body_std": float(wb[h, 0].std()), "pitch_rate_body_std": float(wb[h, 1].std()), "vz_std": float(d[h, 9].std()),
            "vx_body": vb[:, 0]}


def statistics_from_sums(sums):
    """sums [18, n] (STAT_SLOTS) -> dict of [n] arrays: the keys of body_statistics (mean / standard deviation over the accumulated frames), in
    the sums form the device keeps, plus `frames` and `falls`"""
    s = {k: np.asarray(sums[i], np.float64) for i, k in enumerate(STAT_SLOTS)}
    cnt = np.maximum(s["n"], 1.0)
    mean = lambda k: s[k] / cnt
    std = lambda k: np.sqrt(np.maximum(s[k + "2"] / cnt - (s[k] / cnt) ** 2, 0.0))
    return {"vx_body_mean": mean("vx"), "vx_body_std": std("vx"), "vy_body_mean": mean("vy"), "z_mean": mean("z"), "z_std": std("z"), "roll_std": std("roll"),
            "pitch_mean": mean("pitch"), "pitch_std": std("pitch"), "yaw_rate_mean": mean("wz"), "roll_rate_body_std": std("wx"),
            "pitch_rate_body_std": std("wy"), "vz_std": std("vz"), "frames": s["n"].astype(np.int64), "falls": s["falls"].astype(np.int64)}


# ---- the ensemble analysis of a body recorder: entropy, cell counts, histograms, moments per (condition, frame) ----
ENSEMBLE_FEATURES = ("z", "roll", "pitch", "vz_body", "wx_body", "wy_body")
# the cells of Data_Visualization_Code/Figure3.py:361-366 and the density ranges of Figure3.py:198-199, 218 (101 bins)
ENSEMBLE_SPEC_REFERENCE = dict(lb=(0.0, -3.14, -1.57, -10.0, -10.0, -10.0), ub=(0.5, 3.14, 1.57, 10.0, 10.0, 10.0),
                               prec=(0.005, 0.02, 0.02, 0.005, 0.025, 0.025),
                               hist_lo=(0.2, -1.0, -1.0, -5.0, -5.0, -5.0), hist_hi=(0.4, 1.0, 1.0, 5.0, 5.0, 5.0), hist_bins=101)
ENSEMBLE_MAX = 16384          # IRRL_EVAL_ENSEMBLE_MAX
ENSEMBLE_MAX_BINS = 256       # IRRL_EVAL_ENSEMBLE_MAX_BINS
ENSEMBLE_EDGE = 1e-9          # ensemble_edges: how close to a cell boundary (in cells) a sample counts as "on an edge"


def ensemble_spec(spec):
    """a spec mapping (keys of ENSEMBLE_SPEC_REFERENCE; the histogram keys may be left out: no histograms) -> dict of float64 [6] arrays and
    the int hist_bins, refused like irrl_eval_ensemble refuses its struct"""
    s = {k: np.array(spec[k], np.float64).reshape(6) for k in ("lb", "ub", "prec")}
    bins = int(spec.get("hist_bins", 0) or 0)
    for k in ("hist_lo", "hist_hi"):
        s[k] = np.array(spec[k], np.float64).reshape(6) if bins > 0 else np.zeros(6)
    s["hist_bins"] = bins
    if not (np.all(np.isfinite(s["prec"])) and np.all(s["prec"] > 0)):
        raise ValueError("ensemble spec: prec_i > 0")
    if not (np.all(np.isfinite(s["lb"])) and np.all(np.isfinite(s["ub"])) and np.all(s["lb"] <= s["ub"])):
        raise ValueError("ensemble spec: lb_i <= ub_i, both finite")
    if not (np.all(np.abs(s["lb"] / s["prec"]) < 2.0 ** 62) and np.all(np.abs(s["ub"] / s["prec"]) < 2.0 ** 62)):
        raise ValueError("ensemble spec: a bound lies beyond 2^62 cells")
    product = 1
    for r in ensemble_radix(s)[1]:
        product *= int(r)
    if product >= 2 ** 63:
        raise ValueError("ensemble spec: the product of the six cell ranges reaches 2^63: the key does not fit 64 bits")
    if bins < 0 or bins > ENSEMBLE_MAX_BINS:
        raise ValueError("ensemble spec: hist_bins lies in 0 .. %d" % ENSEMBLE_MAX_BINS)
    if bins > 0 and not (np.all(np.isfinite(s["hist_lo"])) and np.all(np.isfinite(s["hist_hi"])) and np.all(s["hist_hi"] > s["hist_lo"])):
        raise ValueError("ensemble spec: hist_lo_i < hist_hi_i, both finite")
    return s


def ensemble_radix(s):
    """-> (lo [6], radix [6]) int64 of a spec: lo_i = trunc(lb_i / prec_i), radix_i = trunc(ub_i / prec_i) - lo_i + 1"""
    lo = (s["lb"] / s["prec"]).astype(np.int64)
    hi = (s["ub"] / s["prec"]).astype(np.int64)
    return lo, hi - lo + 1


def ensemble_features(body):
    """body [..., 13] (a body recorder: base x y z, quaternion w x y z, world linear velocity, world angular velocity) -> x [..., 6] float64 =
    (z, roll, pitch, body-frame v_z, body-frame w_x, body-frame w_y), csrc/eval_elements.hpp irrl_eval_ensemble_features statement for statement
    (the reference's state vector, Figure4.py:98-101, with the rotation matrix of the quaternion itself: the figure script's
    qua2matrix(w, x, x, z) slip is not reproduced)"""
    d = np.asarray(body, np.float32).astype(np.float64)
    pz = d[..., 2]
    w, x, y, z = d[..., 3], d[..., 4], d[..., 5], d[..., 6]
    v0, v1, v2 = d[..., 7], d[..., 8], d[..., 9]
    o0, o1, o2 = d[..., 10], d[..., 11], d[..., 12]
    r00 = 1 - 2 * (y * y + z * z); r01 = 2 * (x * y - w * z); r02 = 2 * (x * z + w * y)
    r10 = 2 * (x * y + w * z); r11 = 1 - 2 * (x * x + z * z); r12 = 2 * (y * z - w * x)
    r20 = 2 * (x * z - w * y); r21 = 2 * (w * x + y * z); r22 = 1 - 2 * (x * x + y * y)
    with np.errstate(invalid="ignore"):
        roll = np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
        sp = 2 * (w * y - x * z)
        sp = np.where(sp > 1.0, 1.0, np.where(sp < -1.0, -1.0, sp))
        pitch = np.arcsin(sp)
        return np.stack([pz, roll, pitch, r02 * v0 + r12 * v1 + r22 * v2, r00 * o0 + r10 * o1 + r20 * o2, r01 * o0 + r11 * o1 + r21 * o2], -1)


def ensemble_keys(x, spec):
    """x [..., 6] -> (key uint64 [...], kept bool [...]): irrl_eval_ensemble_key -- clip, divide by prec, truncate toward zero (astype: the cell
    around 0 is double width), mixed radix with feature 0 the most significant digit; kept is False where a feature is not finite (key 0 there)"""
    s = ensemble_spec(spec)
    x = np.asarray(x, np.float64)
    kept = np.all(np.isfinite(x), -1)
    lo, radix = ensemble_radix(s)
    safe = np.where(kept[..., None], x, 0.0)
    cells = (np.minimum(np.maximum(safe, s["lb"]), s["ub"]) / s["prec"]).astype(np.int64)
    key = np.zeros(x.shape[:-1], np.uint64)
    for i in range(6):
        key = key * np.uint64(radix[i]) + (cells[..., i] - lo[i]).astype(np.uint64)
    return np.where(kept, key, np.uint64(0)), kept


def ensemble_bins(x, lo, hi, bins):
    """irrl_eval_ensemble_bin on an array: floor((x - lo) * (bins / (hi - lo))), x == hi in the last bin, -1 outside [lo, hi] (and for NaN)"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        inside = (x >= lo) & (x <= hi)
        scale = float(bins) / (hi - lo)
        b = np.floor((np.where(inside, x, lo) - lo) * scale).astype(np.int64)
    b = np.minimum(b, bins - 1)
    return np.where(inside, np.where(x == hi, bins - 1, b), -1)


def ensemble_edges(x, spec, tol=ENSEMBLE_EDGE):
    """x [..., 6] -> bool [...]: is the sample "on an edge" of the entropy cells -- an unclipped feature within tol cells of a cell boundary other
    than 0 (truncation has no boundary at 0), or a feature within tol * prec of lb or ub -- so that two correct f64 evaluations of the features
    (different atan2 / asin / fused multiply-adds) may put it into different cells.  Non-finite samples are not on an edge (both sides drop them)."""
    s = ensemble_spec(spec)
    x = np.asarray(x, np.float64)
    fin = np.all(np.isfinite(x), -1, keepdims=True)
    x = np.where(fin, x, 0.5 * (s["lb"] + s["ub"]))
    q = x / s["prec"]
    r = np.round(q)
    inside = (x > s["lb"]) & (x < s["ub"])
    edge = inside & (np.abs(q - r) < tol) & (r != 0)
    edge |= (np.abs(x - s["lb"]) < tol * s["prec"]) | (np.abs(x - s["ub"]) < tol * s["prec"])
    return np.any(edge, -1) & fin[..., 0]


def _ensemble_frames(rows, frame_first, frame_every, frames):
    frame_first, frame_every = int(frame_first), int(frame_every)
    if frame_first < 0 or frame_every < 1:
        raise ValueError("frame_first >= 0, frame_every >= 1")
    most = max(0, -(-(rows - frame_first) // frame_every))
    frames = most if frames is None else int(frames)
    if frames < 0 or frames > most:
        raise ValueError("frame_first + (frames - 1) * frame_every reaches past the recorder's %d rows" % rows)
    return frame_first, frame_every, frames


def _ensemble_shape(n, conditions):
    conditions = int(conditions)
    if conditions < 1 or n % conditions:
        raise ValueError("conditions * explorations != num_envs")
    e = n // conditions
    if e < 1 or e > ENSEMBLE_MAX:
        raise ValueError("explorations lies in 1 .. %d" % ENSEMBLE_MAX)
    return conditions, e


def ensemble_numpy(body, conditions, spec, mask=None, frame_first=0, frame_every=1, frames=None):
    """The float64 twin of irrl_eval_ensemble (include/irrl_env.h): body [rows, N, 13] with env index = condition * E + exploration, analysed
    frame f = row frame_first + f * frame_every (frames None: as many as the rows hold), mask [N] (None: all) -> dict of
    entropy [C, F] f64 (nats), kept / occupied / largest [C, F] uint32, hist [C, F, 6, hist_bins] uint32 (None without bins),
    moments [C, F, 6, 2] f64 (sum x | sum x^2 of the unclipped features over the kept samples)."""
    s = ensemble_spec(spec)
    body = np.asarray(body)
    rows, n = body.shape[0], body.shape[1]
    C_, E = _ensemble_shape(n, conditions)
    frame_first, frame_every, F = _ensemble_frames(rows, frame_first, frame_every, frames)
    bins = s["hist_bins"]
    out = dict(entropy=np.zeros((C_, F)), kept=np.zeros((C_, F), np.uint32), occupied=np.zeros((C_, F), np.uint32), largest=np.zeros((C_, F), np.uint32),
               hist=np.zeros((C_, F, 6, bins), np.uint32) if bins > 0 else None, moments=np.zeros((C_, F, 6, 2)))
    on = np.ones(n, bool) if mask is None else np.asarray(mask).reshape(n) != 0
    for f in range(F):
        x = ensemble_features(body[frame_first + f * frame_every])
        key, kept = ensemble_keys(x, s)
        kept &= on
        for c in range(C_):
            sl = slice(c * E, (c + 1) * E)
            k, xs = key[sl][kept[sl]], x[sl][kept[sl]]
            m = len(k)
            out["kept"][c, f] = m
            out["moments"][c, f, :, 0] = xs.sum(0)
            out["moments"][c, f, :, 1] = (xs * xs).sum(0)
            if bins > 0:
                for i in range(6):
                    b = ensemble_bins(xs[:, i], s["hist_lo"][i], s["hist_hi"][i], bins)
                    out["hist"][c, f, i] = np.bincount(b[b >= 0], minlength=bins)
            if m:
                _, cnt = np.unique(k, return_counts=True)     # sorted keys: the runs in the kernel's order
                p = cnt / float(m)
                out["entropy"][c, f] = -np.sum(p * np.log(p))
                out["occupied"][c, f] = len(cnt)
                out["largest"][c, f] = cnt.max()
    return out


def ensemble_device(rec_body, conditions, spec, mask=None, frame_first=0, frame_every=1, frames=None, hist=True, moments=True):
    """ensemble_numpy on the device: rec_body a float32 device tensor [rows, N, 13] (PolicyEvaluator.run(record=("body",))), mask a uint8 / bool
    device tensor [N] or None -- ONE call of irrl_eval_ensemble on torch's current stream, no synchronisation -> dict of device tensors with the
    twin's keys (hist None with hist=False or without bins, moments None with moments=False)."""
    import torch
    from . import _lib
    from ._lib import ptr
    s = ensemble_spec(spec)
    if rec_body.dim() != 3 or rec_body.shape[2] != 13 or rec_body.dtype != torch.float32 or not rec_body.is_cuda:
        raise ValueError("rec_body is a float32 device tensor [rows, N, 13]")
    rec_body = _lib.contig(rec_body)
    rows, n = int(rec_body.shape[0]), int(rec_body.shape[1])
    C_, E = _ensemble_shape(n, conditions)
    frame_first, frame_every, F = _ensemble_frames(rows, frame_first, frame_every, frames)
    dev = rec_body.device
    if mask is not None:
        mask = _lib.contig(mask.to(device=dev, dtype=torch.uint8).reshape(n))
    bins = s["hist_bins"]
    st = _lib.EvalEnsembleSpec(hist_bins=bins)
    for k in ("lb", "ub", "prec", "hist_lo", "hist_hi"):
        setattr(st, k, (C.c_double * 6)(*s[k]))
    out = dict(entropy=torch.zeros(C_, F, device=dev, dtype=torch.float64), counts=torch.zeros(C_, F, 3, device=dev, dtype=torch.int32),
               hist=torch.zeros(C_, F, 6, bins, device=dev, dtype=torch.int32) if (hist and bins > 0) else None,
               moments=torch.zeros(C_, F, 6, 2, device=dev, dtype=torch.float64) if moments else None)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().irrl_eval_ensemble(ptr(rec_body), rows, n, C_, E, frame_first, frame_every, F, ptr(mask), C.cast(C.pointer(st), C.c_void_p),
                                                  ptr(out["entropy"]), ptr(out["counts"]), ptr(out["hist"]), ptr(out["moments"]), _lib.stream_ptr(dev)))
    counts = out.pop("counts")
    out.update(kept=counts[..., 0], occupied=counts[..., 1], largest=counts[..., 2])
    return out


def ensemble_to_numpy(res):
    """a result of ensemble_device -> the twin's dict of numpy arrays (synchronises; the counters as uint32)"""
    out = {}
    for k, v in res.items():
        a = None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v))
        out[k] = a.astype(np.uint32) if a is not None and k in ("kept", "occupied", "largest", "hist") else a
    return out


def ensemble_row(res, c, control_dt, frame0=0):
    """condition c of an ensemble result (numpy) as perturbation_study hands it out: dict of t [F] (= (frame0 + frame) * control_dt), entropy,
    kept, occupied, largest [F], hist [F, 6, bins] or None, mean and std [F, 6] of the unclipped features over the kept samples (NaN where none)"""
    kept = np.asarray(res["kept"][c], np.float64)
    row = dict(t=(frame0 + np.arange(len(kept))) * float(control_dt), entropy=np.array(res["entropy"][c]), kept=np.array(res["kept"][c]),
               occupied=np.array(res["occupied"][c]), largest=np.array(res["largest"][c]), hist=None if res["hist"] is None else np.array(res["hist"][c]))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = res["moments"][c][:, :, 0] / kept[:, None]
        row["mean"] = mean
        row["std"] = np.sqrt(np.maximum(res["moments"][c][:, :, 1] / kept[:, None] - mean * mean, 0.0))
    return row


def entropy_curve(t, a, b, c, d):
    """the reference's piecewise_func3 (Figure4.py:169-173): the plateau b up to a, slope d up to c, constant d (c - a) + b after"""
    t = np.asarray(t, np.float64)
    return b + d * np.clip(t - a, 0.0, c - a)


def entropy_rate(t, H, stride=1):
    """Least-squares fit of entropy_curve to an entropy series without scipy: every pair a < c out of the frame times t[::stride] is tried, and
    for a pair the curve is b + d g(t) with g = clip(t - a, 0, c - a), linear in (b, d): closed-form least squares, the sums over the frames from
    prefix sums (so the whole grid costs O(n^2) words).  t ascending.  -> dict(a, b, c, d, residual (the root of the mean squared error), kappa
    (= d, nats/s: the entropy's decay rate), t_floor (= c))."""
    t, H = np.asarray(t, np.float64).reshape(-1), np.asarray(H, np.float64).reshape(-1)
    n = len(t)
    if n < 3 or len(H) != n or np.any(np.diff(t) <= 0):
        raise ValueError("entropy_rate needs at least 3 frames and ascending times")
    tm, hm = t.mean(), H.mean()
    tc, hc = t - tm, H - hm                                    # centred: the normal equations lose fewer digits
    pre = lambda v: np.concatenate([[0.0], np.cumsum(v)])
    St, Stt, Sh, Sth = pre(tc), pre(tc * tc), pre(hc), pre(tc * hc)
    idx = np.arange(0, n, max(int(stride), 1))
    i, j = np.meshgrid(idx, idx, indexing="ij")
    ok = i < j
    a, c = tc[i], tc[j]
    mid, tail = (j - i).astype(np.float64), (n - 1 - j).astype(np.float64)
    dt_, dtt, dh, dth = St[j + 1] - St[i + 1], Stt[j + 1] - Stt[i + 1], Sh[j + 1] - Sh[i + 1], Sth[j + 1] - Sth[i + 1]
    sg = dt_ - a * mid + tail * (c - a)
    sgg = dtt - 2 * a * dt_ + a * a * mid + tail * (c - a) ** 2
    sgh = dth - a * dh + (c - a) * (Sh[n] - Sh[j + 1])
    sy, syy = Sh[n], float(np.sum(hc * hc))
    den = n * sgg - sg * sg
    with np.errstate(invalid="ignore", divide="ignore"):
        d = (n * sgh - sg * sy) / den
        b = (sy - d * sg) / n
        sse = syy - b * sy - d * sgh
    sse = np.where(ok & (den > 0), sse, np.inf)
    bi, bj = np.unravel_index(np.argmin(sse), sse.shape)
    a_, c_ = t[idx[bi]], t[idx[bj]]
    g = np.clip(t - a_, 0.0, c_ - a_)                          # the winning pair once more, directly
    gm = g.mean()
    d_ = float(np.sum((g - gm) * (H - hm)) / np.sum((g - gm) ** 2))
    b_ = float(hm - d_ * gm)
    res = float(np.sqrt(np.mean((entropy_curve(t, a_, b_, c_, d_) - H) ** 2)))
    return dict(a=float(a_), b=b_, c=float(c_), d=d_, residual=res, kappa=d_, t_floor=float(c_))


def poincare_section(body_rows, every, offset=0):
    """the strided return map of ONE robot (Figure4.py:191-199: frames offset, offset + every, ... of a run): body_rows [frames, 13] -> the
    features [K, 6] (ENSEMBLE_FEATURES) of those frames; the map's points are (section[:-1], section[1:])"""
    every, offset = int(every), int(offset)
    if every < 1 or offset < 0:
        raise ValueError("every >= 1, offset >= 0")
    return ensemble_features(np.asarray(body_rows)[offset::every])


# ---- the recurrence analysis of a body recorder: the time x time matrix of quantised state distances and its measures per robot ----
# lb, ub, eps, steps: Data_Visualization_Code/Figure4.py:495-509 (the recurrence plot).  radius, theiler, lmin, vmin are THIS build's choices: the
# reference draws the matrix and computes no measures.
RECURRENCE_SPEC_REFERENCE = dict(lb=(0.2, -1.0, -1.0, -5.0, -5.0, -5.0), ub=(0.4, 1.0, 1.0, 5.0, 5.0, 5.0), eps=0.001, steps=40,
                                 radius=10, theiler=10, lmin=2, vmin=2)
RECURRENCE_MAX_FRAMES = 2048     # IRRL_EVAL_RECURRENCE_MAX_FRAMES
RECURRENCE_MAX_MATRICES = 8      # IRRL_EVAL_RECURRENCE_MAX_MATRICES
RECURRENCE_COUNTS = ("kept", "rec", "diag_points", "diag_lines", "diag_max", "vert_points", "vert_lines", "vert_max", "rec_full")
RECURRENCE_EDGE = 1e-9           # recurrence_edges: how close to a level boundary (in levels) a pair counts as "on an edge"


def recurrence_spec(spec):
    """a spec mapping (keys of RECURRENCE_SPEC_REFERENCE) -> dict of the float64 [6] arrays lb, ub, the float eps and the ints steps, radius,
    theiler, lmin, vmin, refused like irrl_eval_recurrence refuses its struct (what depends on the call -- frames, lags, the matrix robots -- is
    refused by the functions that take them)"""
    s = {k: np.array(spec[k], np.float64).reshape(6) for k in ("lb", "ub")}
    s["eps"] = float(spec["eps"])
    for k in ("steps", "radius", "theiler", "lmin", "vmin"):
        s[k] = int(spec[k])
    if not (np.all(np.isfinite(s["lb"])) and np.all(np.isfinite(s["ub"])) and np.all(s["ub"] > s["lb"])):
        raise ValueError("recurrence spec: lb_k < ub_k, both finite")
    if not (np.isfinite(s["eps"]) and s["eps"] > 0):
        raise ValueError("recurrence spec: eps > 0, finite")
    if s["steps"] < 1 or s["steps"] > 255:
        raise ValueError("recurrence spec: steps lies in 1 .. 255")
    if s["radius"] < 1 or s["radius"] > s["steps"]:
        raise ValueError("recurrence spec: radius lies in 1 .. steps")
    if s["theiler"] < 0 or s["lmin"] < 1 or s["vmin"] < 1:
        raise ValueError("recurrence spec: theiler >= 0, lmin >= 1, vmin >= 1")
    return s


def _recurrence_frames(rows, frame_first, frame_every, frames):
    frame_first, frame_every, frames = _ensemble_frames(rows, frame_first, frame_every, frames)
    if frames > RECURRENCE_MAX_FRAMES:
        raise ValueError("frames lies in 0 .. %d" % RECURRENCE_MAX_FRAMES)
    return frame_first, frame_every, frames


def _recurrence_lags(lags, frames):
    lags = frames if lags is None else int(lags)
    if lags < 0 or lags > frames:
        raise ValueError("lags lies in 0 .. frames")
    return lags


def recurrence_states(body, spec, frame_first=0, frame_every=1, frames=None):
    """body [rows, N, 13] -> (u [N, T, 6] float64, kept bool [N, T]): frame i is row frame_first + i * frame_every, x = ensemble_features(row),
    kept iff the six features are finite, u = (x - (lb + ub) / 2.0) / (ub - lb) (irrl_eval_recurrence_state; zeros where dropped)"""
    s = recurrence_spec(spec)
    body = np.asarray(body)
    frame_first, frame_every, T = _recurrence_frames(body.shape[0], frame_first, frame_every, frames)
    x = ensemble_features(body[frame_first:frame_first + T * frame_every:frame_every][:T])
    kept = np.all(np.isfinite(x), -1)
    mid = (s["lb"] + s["ub"]) / 2.0
    width = s["ub"] - s["lb"]
    with np.errstate(over="ignore"):
        u = (np.where(kept[..., None], x, 0.0) - mid) / width
    u = np.where(kept[..., None], u, 0.0)
    return np.ascontiguousarray(u.transpose(1, 0, 2)), np.ascontiguousarray(kept.T)


def _recurrence_distances(u_n):
    """one robot's states [T, 6] -> the f64 distance matrix d = sqrt(d2) [T, T], d2 summed over the features in index order, every product
    rounded on its own (irrl_eval_recurrence_dist2)"""
    T = u_n.shape[0]
    d2 = np.zeros((T, T))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(6):
            delta = u_n[:, None, k] - u_n[None, :, k]
            sq = delta * delta
            d2 = d2 + sq
        return np.sqrt(d2)


def recurrence_levels_numpy(body, spec, frame_first=0, frame_every=1, frames=None):
    """The float64 twin of the element functions of irrl_eval_recurrence (csrc/eval_elements.hpp), statement for statement: body [rows, N, 13] ->
    q uint8 [N, T, T], q_ij = c >= steps ? steps : floor(c) with c = sqrt(d2) / eps, `steps` for a pair with a dropped frame (so the diagonal is
    0 for a kept frame and `steps` for a dropped one: recurrence_kept)"""
    s = recurrence_spec(spec)
    u, kept = recurrence_states(body, s, frame_first, frame_every, frames)
    N, T = kept.shape
    q = np.empty((N, T, T), np.uint8)
    for n in range(N):
        with np.errstate(invalid="ignore", over="ignore"):
            c = _recurrence_distances(u[n]) / s["eps"]
            level = np.where(c < s["steps"], np.floor(np.where(c < s["steps"], c, 0.0)), s["steps"])
        both = kept[n][:, None] & kept[n][None, :]
        q[n] = np.where(both, level, s["steps"]).astype(np.uint8)
    return q


def recurrence_kept(q):
    """q [..., T, T] -> kept bool [..., T]: the diagonal is 0 for a kept frame and `steps` >= 1 for a dropped one"""
    return np.diagonal(np.asarray(q), axis1=-2, axis2=-1) == 0


def recurrence_edges(body, spec, frame_first=0, frame_every=1, frames=None, tol=RECURRENCE_EDGE):
    """body [rows, N, 13] -> bool [N, T, T]: is the pair "on an edge" -- both frames kept and c = d / eps within tol of one of the level boundaries
    1 .. steps (there is none at 0: c >= 0) --, so that two correct f64 evaluations of the features (different atan2 / asin / fused
    multiply-adds) may put it into different levels"""
    s = recurrence_spec(spec)
    u, kept = recurrence_states(body, s, frame_first, frame_every, frames)
    N, T = kept.shape
    out = np.zeros((N, T, T), bool)
    for n in range(N):
        with np.errstate(invalid="ignore", over="ignore"):
            c = _recurrence_distances(u[n]) / s["eps"]
            r = np.round(c)
            out[n] = (np.abs(c - r) < tol) & (r >= 1) & (r <= s["steps"]) & kept[n][:, None] & kept[n][None, :]
    return out


def _run_lengths(flags):
    """a 1-D bool array -> the lengths of its maximal runs of True"""
    d = np.diff(np.concatenate([[0], np.asarray(flags, np.int8), [0]]))
    return np.flatnonzero(d == -1) - np.flatnonzero(d == 1)


def recurrence_from_levels(q, kept, spec, lags=None):
    """The integer stage of the twin: q uint8 [N, T, T] (or [T, T]) and kept bool [N, T] (None: recurrence_kept(q)) -> (counts uint32 [N, 9],
    lag uint32 [N, lags]) as include/irrl_env.h defines them (RECURRENCE_COUNTS; lags None: T).  R_ij = q_ij < radius, w = max(theiler, 1); a
    diagonal line is a maximal run along i of R_{i,i+tau} for a fixed tau >= w, a vertical line a maximal run along i for a fixed j in the full
    matrix with the band |i - j| < w removed; the matrix border ends a line."""
    s = recurrence_spec(spec)
    q = np.asarray(q)
    single = q.ndim == 2
    q = q[None] if single else q
    N, T = q.shape[0], q.shape[1]
    kept = recurrence_kept(q) if kept is None else np.asarray(kept, bool).reshape(N, T)
    lags = _recurrence_lags(lags, T)
    w = max(s["theiler"], 1)
    counts, lag = np.zeros((N, 9), np.uint32), np.zeros((N, lags), np.uint32)
    ii = np.arange(T)
    band = np.abs(ii[:, None] - ii[None, :]) >= w
    for n in range(N):
        R = q[n] < s["radius"]
        for l in range(lags):
            lag[n, l] = np.count_nonzero(np.diagonal(R, l))
        sep = np.zeros(1, bool)
        diag = [np.concatenate([np.diagonal(R, tau), sep]) for tau in range(w, T)]
        runs = _run_lengths(np.concatenate(diag)) if diag else np.zeros(0, np.int64)
        Rb = R & band
        vruns = _run_lengths(np.concatenate([Rb.T, np.zeros((T, 1), bool)], 1).reshape(-1))
        long_d, long_v = runs[runs >= s["lmin"]], vruns[vruns >= s["vmin"]]
        counts[n] = [np.count_nonzero(kept[n]), runs.sum(), long_d.sum(), len(long_d), runs.max() if len(runs) else 0,
                     long_v.sum(), len(long_v), vruns.max() if len(vruns) else 0, np.count_nonzero(Rb)]
    return (counts[0], lag[0]) if single else (counts, lag)


def recurrence_numpy(body, spec, frame_first=0, frame_every=1, frames=None, lags=None, matrix_env=()):
    """The twin of irrl_eval_recurrence, both stages: -> dict(counts uint32 [N, 9], lag uint32 [N, lags] (lags None: T), matrix uint8 [len(matrix_env),
    T, T] -- the levels of the listed robots -- or None)"""
    q = recurrence_levels_numpy(body, spec, frame_first, frame_every, frames)
    counts, lag = recurrence_from_levels(q, None, spec, lags)
    env = _recurrence_matrix_env(matrix_env, q.shape[0])
    return dict(counts=counts, lag=lag, matrix=q[env] if len(env) else None)


def _recurrence_matrix_env(matrix_env, n):
    env = [int(e) for e in matrix_env]
    if len(env) > RECURRENCE_MAX_MATRICES:
        raise ValueError("matrix_count lies in 0 .. %d" % RECURRENCE_MAX_MATRICES)
    if any(e < 0 or e >= n for e in env):
        raise ValueError("a matrix_env lies outside 0 .. num_envs - 1")
    return env


def recurrence_struct(spec, lags=0, matrix_env=()):
    """-> _lib.EvalRecurrenceSpec of a spec, the number of lag words and the robots whose matrices are wanted"""
    from . import _lib
    s = recurrence_spec(spec)
    st = _lib.EvalRecurrenceSpec(eps=s["eps"], lags=int(lags), matrix_count=len(matrix_env), **{k: s[k] for k in ("steps", "radius", "theiler", "lmin", "vmin")})
    st.lb, st.ub = (C.c_double * 6)(*s["lb"]), (C.c_double * 6)(*s["ub"])
    st.matrix_env = (C.c_int * 8)(*(list(matrix_env) + [0] * (8 - len(matrix_env))))
    return st


def recurrence_device(rec_body, spec, frame_first=0, frame_every=1, frames=None, lags=None, matrix_env=()):
    """recurrence_numpy on the device: rec_body a float32 device tensor [rows, N, 13] (PolicyEvaluator.run(record=("body",))) -- ONE call of
    irrl_eval_recurrence on torch's current stream, one workgroup per robot, no synchronisation -> dict of device tensors counts int32 [N, 9]
    (RECURRENCE_COUNTS), lag int32 [N, lags] (lags None: T; None with lags = 0), matrix uint8 [len(matrix_env), T, T] (None without robots)."""
    import torch
    from . import _lib
    from ._lib import ptr
    s = recurrence_spec(spec)
    if rec_body.dim() != 3 or rec_body.shape[2] != 13 or rec_body.dtype != torch.float32 or not rec_body.is_cuda:
        raise ValueError("rec_body is a float32 device tensor [rows, N, 13]")
    rec_body = _lib.contig(rec_body)
    rows, n = int(rec_body.shape[0]), int(rec_body.shape[1])
    frame_first, frame_every, T = _recurrence_frames(rows, frame_first, frame_every, frames)
    lags = _recurrence_lags(lags, T)
    env = _recurrence_matrix_env(matrix_env, n)
    st = recurrence_struct(s, lags, env)
    dev = rec_body.device
    out = dict(counts=torch.zeros(n, 9, device=dev, dtype=torch.int32), lag=torch.zeros(n, lags, device=dev, dtype=torch.int32) if lags > 0 else None,
               matrix=torch.zeros(len(env), T, T, device=dev, dtype=torch.uint8) if env else None)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().irrl_eval_recurrence(ptr(rec_body), rows, n, frame_first, frame_every, T, C.cast(C.pointer(st), C.c_void_p),
                                                    ptr(out["counts"]), ptr(out["lag"]), ptr(out["matrix"]), _lib.stream_ptr(dev)))
    return out


def recurrence_to_numpy(res):
    """a result of recurrence_device -> the twin's dict of numpy arrays (synchronises; the counters as uint32)"""
    out = {}
    for k, v in res.items():
        a = None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v))
        out[k] = a.view(np.uint32) if a is not None and k in ("counts", "lag") and a.dtype == np.int32 else a
    return out


def recurrence_measures(counts, T, spec):
    """counts [..., 9] of T frames -> dict of float64 arrays [...]: RR = REC / points (points = the pairs i < j with j - i >= w, (T - w)(T - w + 1) / 2),
    DET = DIAG_POINTS / REC, L = DIAG_POINTS / DIAG_LINES, LMAX = DIAG_MAX, LAM = VERT_POINTS / REC_FULL, TT = VERT_POINTS / VERT_LINES; NaN
    where a denominator is 0"""
    s = recurrence_spec(spec)
    c = np.asarray(counts).astype(np.float64)
    w = max(s["theiler"], 1)
    points = float(max(int(T) - w, 0) * (max(int(T) - w, 0) + 1) // 2)
    def ratio(a, b):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)
    return dict(RR=ratio(c[..., 1], np.full(c.shape[:-1], points)), DET=ratio(c[..., 2], c[..., 1]), L=ratio(c[..., 2], c[..., 3]), LMAX=c[..., 4],
                LAM=ratio(c[..., 5], c[..., 8]), TT=ratio(c[..., 5], c[..., 6]))


def recurrence_period(lag, T, min_lag, control_dt):
    """lag [..., lags] (the recurrence count per time lag of T frames) -> dict(lag int64 [...], period_s, period_fraction float64 [...]): the
    smallest l >= min_lag that maximises lag[l] / (T - l) -- the stride period where the gait is regular --, l * control_dt and that fraction;
    -1 / NaN / NaN where no lag word lies at or behind min_lag.  Hand in lag words up to about T / 2: at the far end a diagonal has a handful of
    points and its fraction says little."""
    lag = np.asarray(lag).astype(np.float64)
    lags, min_lag = lag.shape[-1], max(int(min_lag), 0)
    if lags <= min_lag:
        shape = lag.shape[:-1]
        return dict(lag=np.full(shape, -1, np.int64), period_s=np.full(shape, np.nan), period_fraction=np.full(shape, np.nan))
    frac = lag[..., min_lag:] / (int(T) - np.arange(min_lag, lags))
    best = np.argmax(frac, -1)                                   # (the first of equal maxima)
    return dict(lag=best + min_lag, period_s=(best + min_lag) * float(control_dt), period_fraction=np.take_along_axis(frac, best[..., None], -1)[..., 0])


def recurrence_row(counts, lag, T, spec, control_dt):
    """one robot's counts [9] and lag [lags] -> what robustness_sweep hands out: dict(RR, DET, L, LMAX, LAM, TT, period_s, period_fraction, kept)"""
    s = recurrence_spec(spec)
    m = recurrence_measures(counts, T, s)
    p = recurrence_period(lag, T, max(s["theiler"], 1), control_dt)
    out = {k: float(v) for k, v in m.items()}
    out.update(period_s=float(p["period_s"]), period_fraction=float(p["period_fraction"]), kept=int(np.asarray(counts)[0]))
    return out


# ---- the footfall analysis of a gait recorder: debounced contact flags, stride statistics, support patterns, leg phases ----
# reach, hold: Data_Visualization_Code/Figure2.py:97-116 (Contact_filtered: a 5-frame moving average cast to bool, then every gap shorter than 10
# frames filled); phase_bins is this build's choice
FOOTFALL_SPEC_REFERENCE = dict(reach=2, hold=10, phase_bins=16)
FOOTFALL_MAX_FRAMES = 16384      # IRRL_EVAL_FOOTFALL_MAX_FRAMES
FOOTFALL_MAX_REACH, FOOTFALL_MAX_HOLD, FOOTFALL_MAX_BINS = 8, 64, 64
FOOTFALL_NONE = 0xFFFFFFFF       # FIRST_TD / LAST_TD without a touchdown
FOOTFALL_COUNTS = ("frames", "raw_stance", "raw_touchdowns", "stance", "touchdowns", "liftoffs", "first_td", "last_td", "stance_phases", "stance_sum",
                   "stance_max", "swing_phases", "swing_sum", "swing_max")
FOOTFALL_LEGS = ("FR", "FL", "HR", "HL")
FOOTFALL_PATTERNS = 8            # robustness_sweep: the rows of the first 8 conditions carry `pattern` (and `hist`)


def footfall_spec(spec):
    """a spec mapping (keys of FOOTFALL_SPEC_REFERENCE) -> dict of ints, refused like irrl_eval_footfall refuses its struct"""
    s = {k: int(spec[k]) for k in ("reach", "hold", "phase_bins")}
    if s["reach"] < 0 or s["reach"] > FOOTFALL_MAX_REACH:
        raise ValueError("footfall spec: reach lies in 0 .. %d" % FOOTFALL_MAX_REACH)
    if s["hold"] < 0 or s["hold"] > FOOTFALL_MAX_HOLD:
        raise ValueError("footfall spec: hold lies in 0 .. %d" % FOOTFALL_MAX_HOLD)
    if s["phase_bins"] < 0 or s["phase_bins"] > FOOTFALL_MAX_BINS:
        raise ValueError("footfall spec: phase_bins lies in 0 .. %d" % FOOTFALL_MAX_BINS)
    return s


def _gait_frames(rows, frame_first, frame_every, frames, most=FOOTFALL_MAX_FRAMES):
    frame_first, frame_every, frames = _ensemble_frames(rows, frame_first, frame_every, frames)
    if frames > most:
        raise ValueError("frames lies in 0 .. %d" % most)
    return frame_first, frame_every, frames


def _gait_window(rec_gait, rec_done, frame_first, frame_every, frames):
    """-> (the analysed rows of the recorder [T, N, 32], T_e int64 [N]): T_e = the first analysed frame with a non-zero rec_done, T if none"""
    rec = np.asarray(rec_gait)
    if rec.ndim != 3 or rec.shape[2] != GAIT_REC_DIM:
        raise ValueError("rec_gait [rows, N, %d]" % GAIT_REC_DIM)
    frame_first, frame_every, T = _gait_frames(rec.shape[0], frame_first, frame_every, frames)
    sel = frame_first + frame_every * np.arange(T)
    te = np.full(rec.shape[1], T, np.int64)
    if rec_done is not None:
        done = np.asarray(rec_done)
        if done.shape != rec.shape[:2]:
            raise ValueError("rec_done [rows, N]")
        dn = done[sel] != 0
        te = np.where(dn.any(0), dn.argmax(0), T).astype(np.int64)
    return rec[sel], te


def footfall_filter_numpy(c, reach, hold):
    """THE FILTER RULE, sequential, statement for statement irrl_eval_footfall_filter (csrc/eval_elements.hpp): c [T] raw flags -> f bool [T]"""
    c = np.asarray(c) != 0
    T, reach, hold = len(c), int(reach), int(hold)
    f = np.zeros(T, bool)
    for k in range(T):
        k0 = k - reach if k - reach > 0 else 0
        k1 = k + reach if k + reach < T - 1 else T - 1
        f[k] = c[k0:k1 + 1].any()
    for j in range(0, T - hold - 1):
        if not f[j] or f[j + 1]:
            continue
        f[j + 1] = f[j + 1:j + hold + 1].any()
    return f


def footfall_fill_end(T, hold, a, b):
    """irrl_eval_footfall_fill_end: the gap between a (the last frame with d in front, -1: none) and b (the first behind, >= T: none) is filled
    for a < k < the value returned"""
    if a < 0 or b >= T or b - a > hold:
        return a + 1
    end = min(b, T - hold)
    return end if end > a + 1 else a + 1


def footfall_filter_closed_numpy(c, reach, hold):
    """the closed form of the rule, as the kernel applies it: the dilation, then every gap of d through footfall_fill_end"""
    c = np.asarray(c) != 0
    T, reach, hold = len(c), int(reach), int(hold)
    d = np.zeros(T, bool)
    for s in range(-reach, reach + 1):
        if s >= 0:
            d[s:] |= c[:T - s] if s < T else False
        else:
            d[:T + s] |= c[-s:] if -s < T else False
    f = d.copy()
    on = np.flatnonzero(d)
    for a, b in zip(on[:-1], on[1:]):
        if b > a + 1:
            f[a + 1:footfall_fill_end(T, hold, int(a), int(b))] = True
    return f


def _footfall_leg(c, f, out):
    """one leg's raw flags c and filtered flags f (bool [T_e]) -> the 14 counters into out; -> the touchdown frames"""
    T = len(c)
    td = np.flatnonzero(~f[:-1] & f[1:]) + 1 if T > 1 else np.zeros(0, np.int64)
    lo = np.flatnonzero(f[:-1] & ~f[1:]) + 1 if T > 1 else np.zeros(0, np.int64)
    out[0], out[1], out[2] = T, int(c.sum()), int((~c[:-1] & c[1:]).sum()) if T > 1 else 0
    out[3], out[4], out[5] = int(f.sum()), len(td), len(lo)
    out[6], out[7] = (int(td[0]), int(td[-1])) if len(td) else (FOOTFALL_NONE, FOOTFALL_NONE)
    at = np.searchsorted(td, lo) - 1                           # a liftoff's stance began at the last touchdown in front of it
    stance = (lo - td[np.maximum(at, 0)])[at >= 0] if len(td) else np.zeros(0, np.int64)
    at = np.searchsorted(lo, td) - 1                           # a touchdown's swing began at the last liftoff in front of it
    swing = (td - lo[np.maximum(at, 0)])[at >= 0] if len(lo) else np.zeros(0, np.int64)
    out[8], out[9], out[10] = len(stance), int(stance.sum()), int(stance.max()) if len(stance) else 0
    out[11], out[12], out[13] = len(swing), int(swing.sum()), int(swing.max()) if len(swing) else 0
    return td


def footfall_numpy(rec_gait, rec_done, spec, frame_first=0, frame_every=1, frames=None):
    """The twin of irrl_eval_footfall (include/irrl_env.h): rec_gait [rows, N, 32], rec_done [rows, N] or None -> dict(counts uint32 [N, 4, 14]
    (FOOTFALL_COUNTS), support uint32 [N, 16], phase uint32 [N, 3, phase_bins] (None with phase_bins = 0), pattern uint8 [T, N]); the filter is
    footfall_filter_numpy, the sequential rule"""
    s = footfall_spec(spec)
    rec, te = _gait_window(rec_gait, rec_done, frame_first, frame_every, frames)
    T, N, bins = rec.shape[0], rec.shape[1], s["phase_bins"]
    counts = np.zeros((N, 4, len(FOOTFALL_COUNTS)), np.uint32)
    support = np.zeros((N, 16), np.uint32)
    phase = np.zeros((N, 3, bins), np.uint32) if bins > 0 else None
    pattern = np.zeros((T, N), np.uint8)
    for e in range(N):
        n = int(te[e])
        c = rec[:n, e, 24:28] != 0
        tds = []
        out = np.zeros(len(FOOTFALL_COUNTS), np.int64)
        for l in range(4):
            f = footfall_filter_numpy(c[:, l], s["reach"], s["hold"])
            tds.append(_footfall_leg(c[:, l], f, out))
            counts[e, l] = out.astype(np.uint32)
            pattern[:n, e] |= (f.astype(np.uint8) << l).astype(np.uint8)
        support[e] = np.bincount(pattern[:n, e], minlength=16)
        if bins > 0 and len(tds[0]) > 1:
            for l in (1, 2, 3):
                at = np.searchsorted(tds[0], tds[l], side="right") - 1
                for t, i in zip(tds[l], at):
                    if i >= 0 and i + 1 < len(tds[0]):
                        a, b = int(tds[0][i]), int(tds[0][i + 1])
                        phase[e, l - 1, (int(t) - a) * bins // (b - a)] += 1
    return dict(counts=counts, support=support, phase=phase, pattern=pattern)


def footfall_struct(spec):
    from . import _lib
    s = footfall_spec(spec)
    return _lib.EvalFootfallSpec(reach=s["reach"], hold=s["hold"], phase_bins=s["phase_bins"])


def _gait_device_args(rec_gait, rec_done):
    import torch
    from . import _lib
    if rec_gait.dim() != 3 or rec_gait.shape[2] != GAIT_REC_DIM or rec_gait.dtype != torch.float32 or not rec_gait.is_cuda:
        raise ValueError("rec_gait is a float32 device tensor [rows, N, %d]" % GAIT_REC_DIM)
    rec_gait = _lib.contig(rec_gait)
    if rec_done is not None:
        if tuple(rec_done.shape) != tuple(rec_gait.shape[:2]) or rec_done.dtype not in (torch.bool, torch.uint8) or rec_done.device != rec_gait.device:
            raise ValueError("rec_done is a bool / uint8 tensor [rows, N] on rec_gait's device")
        rec_done = _lib.contig(rec_done)
    return rec_gait, rec_done


def footfall_device(rec_gait, rec_done, spec, frame_first=0, frame_every=1, frames=None, support=True, phase=True, pattern=True):
    """footfall_numpy on the device: rec_gait a float32 device tensor [rows, N, 32] (PolicyEvaluator.run(record=("gait", "done"))), rec_done the
    bool / uint8 recorder [rows, N] or None -- ONE call of irrl_eval_footfall on torch's current stream, one workgroup per robot, no
    synchronisation -> dict of device tensors counts int32 [N, 4, 14], support int32 [N, 16], phase int32 [N, 3, phase_bins], pattern uint8
    [T, N]; None for an output that is off (support / phase / pattern False, phase_bins = 0)"""
    import torch
    from . import _lib
    from ._lib import ptr
    s = footfall_spec(spec)
    rec_gait, rec_done = _gait_device_args(rec_gait, rec_done)
    rows, n = int(rec_gait.shape[0]), int(rec_gait.shape[1])
    frame_first, frame_every, T = _gait_frames(rows, frame_first, frame_every, frames)
    st = footfall_struct(s)
    dev, bins = rec_gait.device, s["phase_bins"]
    out = dict(counts=torch.zeros(n, 4, len(FOOTFALL_COUNTS), device=dev, dtype=torch.int32),
               support=torch.zeros(n, 16, device=dev, dtype=torch.int32) if support else None,
               phase=torch.zeros(n, 3, bins, device=dev, dtype=torch.int32) if phase and bins > 0 else None,
               pattern=torch.zeros(T, n, device=dev, dtype=torch.uint8) if pattern else None)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().irrl_eval_footfall(ptr(rec_gait), ptr(rec_done), rows, n, frame_first, frame_every, T, C.cast(C.pointer(st), C.c_void_p),
                                                  ptr(out["counts"]), ptr(out["support"]), ptr(out["phase"]), ptr(out["pattern"]), _lib.stream_ptr(dev)))
    return out


def _gait_to_numpy(res, unsigned):
    out = {}
    for k, v in res.items():
        a = None if v is None else (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v))
        out[k] = a.view(np.uint32) if a is not None and k in unsigned and a.dtype == np.int32 else a
    return out


def footfall_to_numpy(res):
    """a result of footfall_device -> the twin's dict of numpy arrays (synchronises; the counters as uint32)"""
    return _gait_to_numpy(res, ("counts", "support", "phase"))


GAIT_PHASE_TOLERANCE = 0.125      # footfall_row: a leg is "with" or "half a stride from" leg 0 within 1 / 8 stride
# the phase lags (in strides) of FL, HR, HL against FR that name a gait
GAIT_LAGS = {"trot": (0.5, 0.5, 0.0), "pace": (0.5, 0.0, 0.5), "bound": (0.0, 0.5, 0.5), "pronk": (0.0, 0.0, 0.0)}


def footfall_row(counts, support, phase, control_dt):
    """one robot's counts [4, 14], support [16] (or None) and phase [3, bins] (or None) -> dict: per leg l duty<l> (STANCE / FRAMES), stride_s<l>
    ((LAST_TD - FIRST_TD) / (TOUCHDOWNS - 1) frames, in seconds), stride_hz<l>, stance_s<l>, swing_s<l> (the mean complete phase), raw_hz<l> (the
    raw flags' touchdown rate, what gait_from_sums calls stride_hz); their means over the legs duty, stride_hz, raw_hz; frames; flight (support[0]
    / FRAMES); lag1 .. lag3, the circular mean of the phase bins' centres of legs 1 .. 3 against leg 0 in strides, 0 <= lag < 1; gait: "trot" /
    "pace" / "bound" / "pronk" where the three lags sit within 1 / 8 stride of the pattern (legs FR, FL, HR, HL: trot has FL and HR half a
    stride from FR and HL with it), else "other".  NaN where a denominator is 0."""
    c = np.asarray(counts).astype(np.int64)
    dt = float(control_dt)
    div = lambda a, b: float(a) / float(b) if b > 0 else float("nan")
    out = {"frames": int(c[0, 0])}
    for l in range(4):
        n, td = int(c[l, 0]), int(c[l, 4])
        out["duty%d" % l] = div(c[l, 3], n)
        out["stride_s%d" % l] = div(c[l, 7] - c[l, 6], td - 1) * dt if td > 1 else float("nan")
        out["stride_hz%d" % l] = 1.0 / out["stride_s%d" % l] if td > 1 and c[l, 7] > c[l, 6] else float("nan")
        out["stance_s%d" % l] = div(c[l, 9], c[l, 8]) * dt
        out["swing_s%d" % l] = div(c[l, 12], c[l, 11]) * dt
        out["raw_hz%d" % l] = div(c[l, 2], n * dt)
    for k in ("duty", "stride_hz", "raw_hz"):
        v = [out["%s%d" % (k, l)] for l in range(4)]
        out[k] = float(np.mean(v))
    out["flight"] = div(np.asarray(support)[0], c[0, 0]) if support is not None else float("nan")
    lags = []
    for l in range(3):
        lag = float("nan")
        if phase is not None:
            h = np.asarray(phase)[l].astype(np.float64)
            if h.sum() > 0:
                ang = 2.0 * np.pi * (np.arange(len(h)) + 0.5) / len(h)
                sx, sy = float((h * np.cos(ang)).sum()), float((h * np.sin(ang)).sum())
                if math.hypot(sx, sy) > 1e-9 * h.sum():
                    lag = (math.atan2(sy, sx) / (2.0 * np.pi) - 0.5 / len(h)) % 1.0
        out["lag%d" % (l + 1)] = lag
        lags.append(lag)
    out["gait"] = "other"
    if not any(x != x for x in lags):
        off = lambda x, y: abs((x - y + 0.5) % 1.0 - 0.5)
        for name, want in GAIT_LAGS.items():
            if all(off(x, y) <= GAIT_PHASE_TOLERANCE for x, y in zip(lags, want)):
                out["gait"] = name
    return out


# ---- the motor plane of a gait recorder: the joints against the motor's torque-speed envelope, the stride-folded loop ----
MOTOR_MAX_FRAMES, MOTOR_MAX_BINS, MOTOR_MAX_PERIOD = 16384, 64, 1024
MOTOR_COUNTS = ("samples", "sat_up", "sat_low", "outside", "motoring", "braking")
MOTOR_KNEE_RATIO = 1.55
_MOTOR_DOUBLES = ("tau_max", "w_crit", "w_max", "knee_ratio", "sat", "t_lo", "t_hi", "w_lo", "w_hi")
_MOTOR_INTS = ("t_bins", "w_bins", "period")


def motor_spec(env_cfg=None, tau_max=None, w_crit=None, w_max=None, knee_ratio=MOTOR_KNEE_RATIO, sat=0.01, t_lo=-20.0, t_hi=20.0, w_lo=-45.0, w_hi=45.0,
               t_bins=40, w_bins=45, period=100):
    """The spec of irrl_eval_motor_plane.  env_cfg: the `environment:` mapping of a config (MotorMaxTorque, MotorCriticalSpeed, MotorMaxSpeed: the
    envelope the env's torque clamp applies) or None with the three given; sat: how close to the envelope (N m, motor side) a sample counts as
    saturated; the ranges +-20 N m x +-45 rad/s are the axes of the reference's Figure 5, the period its phase_jagged fold's 100 frames.
    -> dict, refused like the C call refuses its struct"""
    cfg = {} if env_cfg is None else dict(env_cfg.get("environment", env_cfg))
    pick = lambda v, key: float(cfg[key]) if v is None else float(v)
    return motor_spec_check(dict(tau_max=pick(tau_max, "MotorMaxTorque"), w_crit=pick(w_crit, "MotorCriticalSpeed"), w_max=pick(w_max, "MotorMaxSpeed"),
                                 knee_ratio=knee_ratio, sat=sat, t_lo=t_lo, t_hi=t_hi, w_lo=w_lo, w_hi=w_hi, t_bins=t_bins, w_bins=w_bins, period=period))


def motor_spec_check(spec):
    s = {k: float(spec[k]) for k in _MOTOR_DOUBLES}
    s.update({k: int(spec[k]) for k in _MOTOR_INTS})
    fin = math.isfinite
    if not fin(s["tau_max"]) or not s["tau_max"] > 0.0:
        raise ValueError("motor spec: tau_max > 0, finite")
    if not fin(s["w_crit"]) or not fin(s["w_max"]) or not s["w_max"] > s["w_crit"]:
        raise ValueError("motor spec: w_crit < w_max, both finite")
    if not fin(s["knee_ratio"]) or not s["knee_ratio"] > 0.0:
        raise ValueError("motor spec: knee_ratio > 0, finite")
    if not fin(s["sat"]) or not s["sat"] >= 0.0:
        raise ValueError("motor spec: sat >= 0, finite")
    if not 0 <= s["t_bins"] <= MOTOR_MAX_BINS or not 0 <= s["w_bins"] <= MOTOR_MAX_BINS:
        raise ValueError("motor spec: t_bins, w_bins lie in 0 .. %d" % MOTOR_MAX_BINS)
    if not 0 <= s["period"] <= MOTOR_MAX_PERIOD:
        raise ValueError("motor spec: period lies in 0 .. %d" % MOTOR_MAX_PERIOD)
    if s["t_bins"] > 0 and s["w_bins"] > 0:
        if not (fin(s["t_lo"]) and fin(s["t_hi"]) and s["t_hi"] > s["t_lo"]) or not (fin(s["w_lo"]) and fin(s["w_hi"]) and s["w_hi"] > s["w_lo"]):
            raise ValueError("motor spec: t_lo < t_hi, w_lo < w_hi, all finite")
    return s


def motor_up(w, s):
    """irrl_eval_motor_up on an array, statement for statement"""
    span = s["w_max"] - s["w_crit"]
    slope = s["tau_max"] / span
    over = w - s["w_crit"]
    drop = over * slope
    return np.where(w > s["w_crit"], s["tau_max"] - drop, s["tau_max"])


def motor_samples(rec, spec):
    """recorder rows [..., 32] -> (m, w float64 [..., 12], kept bool [..., 12]): irrl_eval_motor_sample"""
    ratio = np.where(np.arange(12) % 3 == 2, spec["knee_ratio"], 1.0)
    rec = np.asarray(rec)
    with np.errstate(invalid="ignore", over="ignore"):
        m = rec[..., 0:12].astype(np.float64) / ratio
        w = rec[..., 12:24].astype(np.float64) * ratio
    return m, w, np.isfinite(m) & np.isfinite(w)


def _motor_shape(n, conditions):
    conditions = int(conditions)
    if conditions < 1 or n % conditions:
        raise ValueError("conditions * robots == num_envs, conditions >= 1")
    return conditions, n // conditions


def motor_plane_numpy(rec_gait, rec_done, spec, conditions=None, frame_first=0, frame_every=1, frames=None):
    """The twin of irrl_eval_motor_plane (include/irrl_env.h): rec_gait [rows, N, 32], rec_done [rows, N] or None, env = condition * robots +
    robot (conditions None: N, one robot each) -> dict(counts uint32 [C, 12, 6] (MOTOR_COUNTS), hist uint32 [C, 12, t_bins, w_bins] (None with a
    zero bin count), fold float64 [C, 12, period, 3] (None with period = 0): count, sum m, sum w per phase, added robot by robot and frame by
    frame in index order)"""
    s = motor_spec_check(spec)
    rec, te = _gait_window(rec_gait, rec_done, frame_first, frame_every, frames)
    T, N = rec.shape[0], rec.shape[1]
    Cn, R = _motor_shape(N, N if conditions is None else conditions)
    m, w, kept = motor_samples(rec, s)                         # [T, N, 12]
    kept &= (np.arange(T)[:, None] < te[None, :])[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        up, low = motor_up(w, s), -motor_up(-w, s)
        power = m * w
        classes = [kept, kept & (m >= up - s["sat"]), kept & (m <= low + s["sat"]), kept & ((m > up + s["sat"]) | (m < low - s["sat"])),
                   kept & (power > 0.0), kept & (power < 0.0)]
    counts = np.stack([k.reshape(T, Cn, R, 12).sum((0, 2)) for k in classes], -1).astype(np.uint32)
    hist = fold = None
    tb, wb, period = s["t_bins"], s["w_bins"], s["period"]
    if tb > 0 and wb > 0:
        bt, bw = ensemble_bins(m, s["t_lo"], s["t_hi"], tb), ensemble_bins(w, s["w_lo"], s["w_hi"], wb)
        ok = kept & (bt >= 0) & (bw >= 0)
        cj = (np.arange(N) // R)[None, :, None] * 12 + np.arange(12)[None, None, :]
        cell = (cj * tb + bt) * wb + bw
        hist = np.bincount(cell[ok], minlength=Cn * 12 * tb * wb).astype(np.uint32).reshape(Cn, 12, tb, wb)
    if period > 0:
        K = -(-T // period)
        pad = K * period - T
        z = lambda a: np.concatenate([np.where(kept, a, 0.0), np.zeros((pad, N, 12))], 0).reshape(K, period, Cn, R, 12)
        one, mm, ww = z(np.ones_like(m)), z(m), z(w)
        fold = np.zeros((Cn, 12, period, 3))
        for r in range(R):                                     # robots in order, frames in order: ONE order of the f64 additions
            for k in range(K):
                for i, a in enumerate((one, mm, ww)):
                    fold[:, :, :, i] = fold[:, :, :, i] + a[k, :, :, r, :].transpose(1, 2, 0)
    return dict(counts=counts, hist=hist, fold=fold)


def motor_struct(spec):
    from . import _lib
    s = motor_spec_check(spec)
    return _lib.EvalMotorSpec(**s)


def motor_plane_device(rec_gait, rec_done, spec, conditions=None, frame_first=0, frame_every=1, frames=None, hist=True, fold=True):
    """motor_plane_numpy on the device: ONE call of irrl_eval_motor_plane on torch's current stream, one workgroup per (condition, joint), no
    synchronisation -> dict of device tensors counts int32 [C, 12, 6], hist int32 [C, 12, t_bins, w_bins], fold float64 [C, 12, period, 3]; None
    for an output that is off"""
    import torch
    from . import _lib
    from ._lib import ptr
    s = motor_spec_check(spec)
    rec_gait, rec_done = _gait_device_args(rec_gait, rec_done)
    rows, n = int(rec_gait.shape[0]), int(rec_gait.shape[1])
    Cn, R = _motor_shape(n, n if conditions is None else conditions)
    frame_first, frame_every, T = _gait_frames(rows, frame_first, frame_every, frames, MOTOR_MAX_FRAMES)
    st = motor_struct(s)
    dev = rec_gait.device
    out = dict(counts=torch.zeros(Cn, 12, len(MOTOR_COUNTS), device=dev, dtype=torch.int32),
               hist=torch.zeros(Cn, 12, s["t_bins"], s["w_bins"], device=dev, dtype=torch.int32) if hist and s["t_bins"] > 0 and s["w_bins"] > 0 else None,
               fold=torch.zeros(Cn, 12, s["period"], 3, device=dev, dtype=torch.float64) if fold and s["period"] > 0 else None)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().irrl_eval_motor_plane(ptr(rec_gait), ptr(rec_done), rows, n, Cn, R, frame_first, frame_every, T,
                                                     C.cast(C.pointer(st), C.c_void_p), ptr(out["counts"]), ptr(out["hist"]), ptr(out["fold"]),
                                                     _lib.stream_ptr(dev)))
    return out


def motor_plane_to_numpy(res):
    """a result of motor_plane_device -> the twin's dict of numpy arrays (synchronises; the counters as uint32)"""
    return _gait_to_numpy(res, ("counts", "hist"))


def motor_plane_row(counts):
    """one condition's counts [12, 6] -> dict of float64 [12] arrays: saturated ((SAT_UP + SAT_LOW) / SAMPLES), outside, motoring, braking (NaN
    for a joint without a sample), and samples int64 [12]"""
    c = np.asarray(counts).astype(np.float64)
    n = np.where(c[:, 0] > 0, c[:, 0], np.nan)
    return dict(saturated=(c[:, 1] + c[:, 2]) / n, outside=c[:, 3] / n, motoring=c[:, 4] / n, braking=c[:, 5] / n, samples=np.asarray(counts)[:, 0].astype(np.int64))


# ---- correlation moments of two recorder windows (irrl_eval_correlation) ----
CORR_MAX_FRAMES = 16384          # IRRL_EVAL_CORR_MAX_FRAMES
CORR_MAX_X = 64                  # IRRL_EVAL_CORR_MAX_X
CORR_MAX_Y = 1024                # IRRL_EVAL_CORR_MAX_Y
CORR_MATRICES = 8                # robustness_sweep: the rows of the first 8 conditions carry the [cx, cy] matrix
TRACE_RECORDERS = ("lstm", "value")     # PolicyEvaluator.run: what only the five-launch form records (include/irrl_env.h irrl_eval_trace)
# name -> (recorder of PolicyEvaluator.run, first column, count); lstm's count is the policy's 4 * hid (c0 | h0 | c1 | h1), value's recorder is
# [steps, N], a single column
CORR_SOURCES = {"contact": ("gait", 24, 4), "torque": ("gait", 0, 12), "joint_rate": ("gait", 12, 12), "body": ("body", 0, 13),
                "obs": ("obs_cond", 0, 35), "action": ("act_applied", 0, 12), "lstm": ("lstm", 0, None), "value": ("value", 0, 1)}
_CORR_KEYS = ("x_dim", "x_first", "x_count", "y_dim", "y_first", "y_count")


def correlation_source(name, hid=None):
    """a name out of CORR_SOURCES -> (recorder, row width, first column, count); hid: the policy's LSTM units, needed for "lstm\""""
    if name not in CORR_SOURCES:
        raise KeyError("unknown correlation source %r: choose from %s" % (name, sorted(CORR_SOURCES)))
    rec, first, count = CORR_SOURCES[name]
    if rec == "lstm":
        if hid is None:
            raise ValueError("the correlation source 'lstm' needs the policy's number of LSTM units")
        return rec, 4 * int(hid), first, 4 * int(hid)
    width = GAIT_REC_DIM if rec == "gait" else 1 if rec == "value" else RECORDERS[rec]
    return rec, width, first, count


def correlation_spec(x_dim, x_first, x_count, y_dim, y_first, y_count):
    """The spec of irrl_eval_correlation: of rows x_dim (y_dim) floats wide the columns x_first .. x_first + x_count (y_first ..) are analysed.
    -> dict, refused like the C call refuses its struct"""
    s = dict(zip(_CORR_KEYS, (int(v) for v in (x_dim, x_first, x_count, y_dim, y_first, y_count))))
    if s["x_dim"] < 1 or s["y_dim"] < 1:
        raise ValueError("correlation spec: x_dim >= 1, y_dim >= 1")
    if not 1 <= s["x_count"] <= CORR_MAX_X:
        raise ValueError("correlation spec: x_count lies in 1 .. %d" % CORR_MAX_X)
    if not 1 <= s["y_count"] <= CORR_MAX_Y:
        raise ValueError("correlation spec: y_count lies in 1 .. %d" % CORR_MAX_Y)
    for k in "xy":
        if s[k + "_first"] < 0 or s[k + "_first"] + s[k + "_count"] > s[k + "_dim"]:
            raise ValueError("correlation spec: the %s window lies outside the row width" % k)
    return s


def _corr_frames(rows, frame_first, frame_every, frames):
    frame_first, frame_every, T = _gait_frames(rows, frame_first, frame_every, frames, CORR_MAX_FRAMES)
    if T < 1:
        raise ValueError("frames lies in 1 .. %d" % CORR_MAX_FRAMES)
    return frame_first, frame_every, T


def correlation_numpy(x, y, rec_done, spec, conditions=None, frame_first=0, frame_every=1, frames=None):
    """The twin of irrl_eval_correlation (include/irrl_env.h): x [rows, N, x_dim] and y [rows, N, y_dim] float32 ([rows, N] with a row width of 1),
    rec_done [rows, N] or None, env = condition * robots + robot (conditions None: N, one robot each) -> dict(count int64 [G], sx float64
    [G, cx, 2] (sum x, sum x^2), sy float64 [G, cy, 2], sxy float64 [G, cx, cy], range_x float32 [G, cx, 2] and range_y float32 [G, cy, 2] (min,
    max; +inf, -inf without a sample)) over the frames i < T_e of each condition's robots.  An explicit loop over the frames, every robot and
    pair at once, as s = s + (double)a * (double)b from +0.0, then an explicit loop over a condition's robots from +0.0: the one order of the f64
    additions the kernel and the host program follow, so equal means equal bits.  A NaN sample never enters a range and poisons the sums of
    its own column (pairs) only."""
    s = correlation_spec(**spec)
    cx, cy = s["x_count"], s["y_count"]

    def rows3(a, dim, what):
        a = np.asarray(a)
        a = a[:, :, None] if a.ndim == 2 and dim == 1 else a
        if a.ndim != 3 or a.shape[2] != dim or a.dtype != np.float32:
            raise ValueError("%s: float32 [rows, N, %d]" % (what, dim))
        return a
    x, y = rows3(x, s["x_dim"], "x"), rows3(y, s["y_dim"], "y")
    if x.shape[:2] != y.shape[:2]:
        raise ValueError("x and y have the same rows and N")
    rows, N = x.shape[:2]
    Cn, R = _motor_shape(N, N if conditions is None else conditions)
    frame_first, frame_every, T = _corr_frames(rows, frame_first, frame_every, frames)
    sel = frame_first + frame_every * np.arange(T)
    te = np.full(N, T, np.int64)
    if rec_done is not None:
        done = np.asarray(rec_done)
        if done.shape != (rows, N):
            raise ValueError("rec_done [rows, N]")
        dn = done[sel] != 0
        te = np.where(dn.any(0), dn.argmax(0), T).astype(np.int64)
    xw, yw = x[sel][:, :, s["x_first"]:s["x_first"] + cx], y[sel][:, :, s["y_first"]:s["y_first"] + cy]     # float32 [T, N, c]
    sxy, sx, sy = np.zeros((N, cx, cy)), np.zeros((N, cx, 2)), np.zeros((N, cy, 2))
    inf = np.float32(np.inf)
    rx, ry = np.empty((N, cx, 2), np.float32), np.empty((N, cy, 2), np.float32)
    rx[..., 0] = ry[..., 0] = inf
    rx[..., 1] = ry[..., 1] = -inf
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(int(te.max()) if N else 0):             # frames in ascending order
            on = i < te
            a32, b32 = xw[i], yw[i]
            a, b = a32.astype(np.float64), b32.astype(np.float64)
            sxy = np.where(on[:, None, None], sxy + a[:, :, None] * b[:, None, :], sxy)
            for acc, v, v32, rng in ((sx, a, a32, rx), (sy, b, b32, ry)):
                m = on[:, None]
                acc[..., 0] = np.where(m, acc[..., 0] + v, acc[..., 0])
                acc[..., 1] = np.where(m, acc[..., 1] + v * v, acc[..., 1])
                rng[..., 0] = np.where(m & (v32 < rng[..., 0]), v32, rng[..., 0])
                rng[..., 1] = np.where(m & (v32 > rng[..., 1]), v32, rng[..., 1])
        out = dict(count=te.reshape(Cn, R).sum(1).astype(np.int64))
        for k, part in (("sx", sx), ("sy", sy), ("sxy", sxy)):
            part = part.reshape((Cn, R) + part.shape[1:])
            tot = np.zeros((Cn,) + part.shape[2:])
            for r in range(R):                                 # robots in ascending order
                tot = tot + part[:, r]
            out[k] = tot
        for k, part in (("range_x", rx), ("range_y", ry)):
            part = part.reshape((Cn, R) + part.shape[1:])
            tot = part[:, 0].copy()
            for r in range(1, R):
                tot[..., 0] = np.where(part[:, r, :, 0] < tot[..., 0], part[:, r, :, 0], tot[..., 0])
                tot[..., 1] = np.where(part[:, r, :, 1] > tot[..., 1], part[:, r, :, 1], tot[..., 1])
            out[k] = tot
    return out


def correlation_struct(spec):
    from . import _lib
    return _lib.EvalCorrSpec(**correlation_spec(**spec))


def correlation_work(num_envs, spec):
    """the doubles of `work` for a pool of num_envs: irrl_eval_correlation_work = num_envs * (cx cy + 3 cx + 3 cy + 1)"""
    s = correlation_spec(**spec)
    return int(num_envs) * (s["x_count"] * s["y_count"] + 3 * s["x_count"] + 3 * s["y_count"] + 1)


def correlation_device(x, y, rec_done, spec, conditions=None, frame_first=0, frame_every=1, frames=None, ranges=True, work="auto"):
    """correlation_numpy on the device: ONE call of irrl_eval_correlation on torch's current stream (one workgroup per robot and, with more than
    one robot per condition, a second launch that adds the robots' partials in order), no synchronisation.  x, y: float32 device tensors [rows,
    N, dim] ([rows, N] with a row width of 1; the same tensor for an auto-covariance), rec_done a bool / uint8 device tensor [rows, N] or None.
    work: "auto" = allocated here where robots > 1, None = NULL (one robot per condition only), or a float64 device tensor of correlation_work
    doubles.  -> dict of device tensors count int64 [G], sx, sy, sxy float64, range_x, range_y float32 (None with ranges=False)"""
    import torch
    from . import _lib
    from ._lib import ptr
    s = correlation_spec(**spec)
    cx, cy = s["x_count"], s["y_count"]

    def rows3(a, dim, what):
        a = a.unsqueeze(2) if a.dim() == 2 and dim == 1 else a
        if a.dim() != 3 or a.shape[2] != dim or a.dtype != torch.float32 or not a.is_cuda:
            raise ValueError("%s: a float32 device tensor [rows, N, %d]" % (what, dim))
        return _lib.contig(a)
    x, y = rows3(x, s["x_dim"], "x"), rows3(y, s["y_dim"], "y")
    if x.shape[:2] != y.shape[:2] or x.device != y.device:
        raise ValueError("x and y have the same rows and N and live on one device")
    rows, n = int(x.shape[0]), int(x.shape[1])
    if rec_done is not None:
        if tuple(rec_done.shape) != (rows, n) or rec_done.device != x.device or rec_done.dtype not in (torch.bool, torch.uint8):
            raise ValueError("rec_done: a bool / uint8 device tensor [rows, N]")
        rec_done = _lib.contig(rec_done).view(torch.uint8)
    Cn, R = _motor_shape(n, n if conditions is None else conditions)
    frame_first, frame_every, T = _corr_frames(rows, frame_first, frame_every, frames)
    dev = x.device
    if isinstance(work, str) and work == "auto":
        work = torch.empty(correlation_work(n, s), device=dev, dtype=torch.float64) if R > 1 else None
    elif work is not None and (work.dtype != torch.float64 or work.numel() < correlation_work(n, s) or work.device != dev or not work.is_contiguous()):
        raise ValueError("work: a contiguous float64 device tensor of at least %d elements" % correlation_work(n, s))
    st = correlation_struct(s)
    f64 = dict(device=dev, dtype=torch.float64)
    out = dict(count=torch.zeros(Cn, device=dev, dtype=torch.int64), sx=torch.zeros(Cn, cx, 2, **f64), sy=torch.zeros(Cn, cy, 2, **f64),
               sxy=torch.zeros(Cn, cx, cy, **f64),
               range_x=torch.zeros(Cn, cx, 2, device=dev, dtype=torch.float32) if ranges else None,
               range_y=torch.zeros(Cn, cy, 2, device=dev, dtype=torch.float32) if ranges else None)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().irrl_eval_correlation(ptr(x), ptr(y), ptr(rec_done), rows, n, Cn, R, frame_first, frame_every, T,
                                                     C.cast(C.pointer(st), C.c_void_p), ptr(out["count"]), ptr(out["sx"]), ptr(out["sy"]), ptr(out["sxy"]),
                                                     ptr(out["range_x"]), ptr(out["range_y"]), ptr(work), _lib.stream_ptr(dev)))
    return out


def correlation_to_numpy(res):
    """a result of correlation_device -> the twin's dict of numpy arrays (synchronises)"""
    return {k: None if v is None else v.cpu().numpy() for k, v in res.items()}


def correlation_from_moments(m):
    """The moments of correlation_numpy / correlation_to_numpy -> dict(r [G, cx, cy] the Pearson correlation, cov [G, cx, cy] the sample
    covariance (n - 1 in the denominator, like pandas), mean_x [G, cx], mean_y [G, cy], std_x, std_y (n - 1), count [G]).  r is NaN where the
    condition has fewer than 2 samples or either column is constant -- decided EXACTLY from the ranges, min == max, where they are given (a foot
    that never touches down: pandas gives NaN there too), from a variance that is not positive otherwise; cov and the standard deviations are NaN
    below 2 samples, the means below 1.  The one function behind both the device path and the twin; the differences n sxy - sx sy are taken
    in extended precision."""
    ld = np.longdouble
    n = np.asarray(m["count"]).astype(ld)
    sx1, sx2 = np.asarray(m["sx"])[..., 0].astype(ld), np.asarray(m["sx"])[..., 1].astype(ld)
    sy1, sy2 = np.asarray(m["sy"])[..., 0].astype(ld), np.asarray(m["sy"])[..., 1].astype(ld)
    sxy = np.asarray(m["sxy"]).astype(ld)
    n1, n2, n3 = n[:, None], n[:, None, None], (n * (n - 1))[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cxy = n2 * sxy - sx1[:, :, None] * sy1[:, None, :]
        vx, vy = n1 * sx2 - sx1 * sx1, n1 * sy2 - sy1 * sy1
        r = cxy / np.sqrt(vx[:, :, None] * vy[:, None, :])
        cov = cxy / n3
        few1, few2 = (n < 1), (n < 2)
        if m.get("range_x") is not None and m.get("range_y") is not None:
            flat_x = ~(np.asarray(m["range_x"])[..., 0] < np.asarray(m["range_x"])[..., 1])
            flat_y = ~(np.asarray(m["range_y"])[..., 0] < np.asarray(m["range_y"])[..., 1])
        else:
            flat_x, flat_y = ~(vx > 0), ~(vy > 0)
        bad = few2[:, None, None] | flat_x[:, :, None] | flat_y[:, None, :]
        r = np.where(bad, np.nan, np.clip(r, -1.0, 1.0)).astype(np.float64)
        cov = np.where(few2[:, None, None], np.nan, cov).astype(np.float64)
        mean_x, mean_y = np.where(few1[:, None], np.nan, sx1 / n1).astype(np.float64), np.where(few1[:, None], np.nan, sy1 / n1).astype(np.float64)
        d = (n * (n - 1))[:, None]
        std_x = np.where(few2[:, None], np.nan, np.sqrt(np.maximum(vx, 0) / d)).astype(np.float64)
        std_y = np.where(few2[:, None], np.nan, np.sqrt(np.maximum(vy, 0) / d)).astype(np.float64)
    return dict(r=r, cov=cov, mean_x=mean_x, mean_y=mean_y, std_x=std_x, std_y=std_y, count=np.asarray(m["count"]).astype(np.int64))


def correlation_unit(y_name, j, cy):
    """column j of a y window of cy columns -> for "lstm" (layer 1 or 2, "c" or "h", index) in the recorder's order c0 | h0 | c1 | h1
    (the reference's layer1_c | layer1_h | layer2_c | layer2_h), else (y_name, j)"""
    if y_name != "lstm":
        return (y_name, int(j))
    hid = cy // 4
    block = int(j) // hid
    return (block // 2 + 1, "ch"[block % 2], int(j) % hid)


def correlation_row(m, names, g=0):
    """one condition of the moments -> dict(corr_max: the largest |r| over the [cx, cy] pairs (NaN if no pair has an r), corr_r: that r with its
    sign, corr_leg: the x column's label -- the leg's name out of FOOTFALL_LEGS for the source "contact", else (x name, column) --, corr_unit:
    correlation_unit of the y column).  names: the (x, y) source names out of CORR_SOURCES"""
    x_name, y_name = names
    r = correlation_from_moments({k: None if v is None else np.asarray(v)[g:g + 1] for k, v in m.items()})["r"][0]
    if not np.any(np.isfinite(r)):
        return dict(corr_max=float("nan"), corr_r=float("nan"), corr_leg=None, corr_unit=None)
    i, j = np.unravel_index(int(np.nanargmax(np.abs(r))), r.shape)
    leg = FOOTFALL_LEGS[i] if x_name == "contact" else (x_name, int(i))
    return dict(corr_max=float(abs(r[i, j])), corr_r=float(r[i, j]), corr_leg=leg, corr_unit=correlation_unit(y_name, j, r.shape[1]))


# ---- spectrogram and Welch spectrum of recorder columns (irrl_eval_spectrum) ----
SPECTRUM_MAX_FRAMES = 16384      # IRRL_EVAL_SPECTRUM_MAX_FRAMES
SPECTRUM_MAX_X = 64              # IRRL_EVAL_SPECTRUM_MAX_X
SPECTRUM_MAX_NPERSEG = 1024      # IRRL_EVAL_SPECTRUM_MAX_NPERSEG
SPECTRUM_MAX_MATRICES = 8        # IRRL_EVAL_SPECTRUM_MAX_MATRICES; robustness_sweep: the rows of the first 8 conditions carry the spectrogram
SPECTRUM_WINDOWS = {"boxcar": 0, "hann": 1, "tukey": 2}      # the window_kind of irrl_eval_spectrum_tables
# name -> (recorder of PolicyEvaluator.run, first column, count): what the reference's --virba plots (run_bp_v5.py:1090-1117)
SPECTRUM_SOURCES = {"joint": ("obs_cond", 5, 12), "joint_rate": ("obs_cond", 17, 12), "action": ("act_applied", 0, 12)}
# the reference's bare scipy.signal.spectrogram(column, fs): Tukey(0.25), 256 frames per segment, 32 of them shared, a constant detrend; and the
# 50 Hz of its set_ylim([0, 50]) as the band above which power counts as vibration
SPECTRUM_REFERENCE = dict(nperseg=256, hop=224, window="tukey", alpha=0.25, detrend=1, band_hz=50.0)


def spectrum_spec(x_dim, x_first, x_count, nperseg, hop, fs, scale=None, detrend=1, matrix_env=()):
    """The spec of irrl_eval_spectrum: of rows x_dim floats wide the columns x_first .. x_first + x_count are analysed in segments of nperseg
    frames, hop frames apart, sampled at fs Hz; scale: one factor per analysed column (None: 1.0), detrend: 1 subtracts each segment's mean,
    matrix_env: up to 8 robots whose spectrograms are wanted.  -> dict, refused like the C call refuses its struct"""
    s = dict(x_dim=int(x_dim), x_first=int(x_first), x_count=int(x_count), nperseg=int(nperseg), hop=int(hop), fs=float(fs), detrend=int(detrend),
             matrix_env=tuple(int(e) for e in matrix_env))
    if s["x_dim"] < 1:
        raise ValueError("spectrum spec: x_dim >= 1")
    if not 1 <= s["x_count"] <= SPECTRUM_MAX_X:
        raise ValueError("spectrum spec: x_count lies in 1 .. %d" % SPECTRUM_MAX_X)
    if s["x_first"] < 0 or s["x_first"] + s["x_count"] > s["x_dim"]:
        raise ValueError("spectrum spec: the x window lies outside the row width")
    if not 8 <= s["nperseg"] <= SPECTRUM_MAX_NPERSEG:
        raise ValueError("spectrum spec: nperseg lies in 8 .. %d" % SPECTRUM_MAX_NPERSEG)
    if not 1 <= s["hop"] <= s["nperseg"]:
        raise ValueError("spectrum spec: hop lies in 1 .. nperseg")
    if s["detrend"] not in (0, 1):
        raise ValueError("spectrum spec: detrend lies in 0 .. 1")
    if not (math.isfinite(s["fs"]) and s["fs"] > 0):
        raise ValueError("spectrum spec: fs > 0, finite")
    sc = np.ones(s["x_count"]) if scale is None else np.asarray(scale, np.float64).reshape(-1)
    if sc.shape != (s["x_count"],) or not np.all(np.isfinite(sc) & (sc > 0)):
        raise ValueError("spectrum spec: scale holds x_count factors > 0, finite")
    s["scale"] = tuple(float(v) for v in sc)
    if len(s["matrix_env"]) > SPECTRUM_MAX_MATRICES:
        raise ValueError("spectrum spec: matrix_env lists at most %d robots" % SPECTRUM_MAX_MATRICES)
    return s


def spectrum_bins(nperseg):
    return int(nperseg) // 2 + 1


def spectrum_frequencies(nperseg, fs):
    """the frequency of every bin, k fs / nperseg (scipy's rfftfreq)"""
    return np.arange(spectrum_bins(nperseg)) * (float(fs) / int(nperseg))


def spectrum_tables(nperseg, window="tukey", alpha=0.25):
    """-> (window float64 [nperseg], tw float64 [nperseg, 2] = cos, sin of 2 pi j / nperseg), filled by the library's host helper
    irrl_eval_spectrum_tables (no GPU): the device call, the twin, the host program and the tests all read THESE bits, so the tables' rounding
    drops out of every comparison.  window: a name out of SPECTRUM_WINDOWS; alpha: Tukey's taper fraction"""
    from . import _lib
    if window not in SPECTRUM_WINDOWS:
        raise KeyError("unknown window %r: choose from %s" % (window, sorted(SPECTRUM_WINDOWS)))
    nperseg = int(nperseg)
    if not 8 <= nperseg <= SPECTRUM_MAX_NPERSEG:
        raise ValueError("nperseg lies in 8 .. %d" % SPECTRUM_MAX_NPERSEG)
    win, tw = np.zeros(nperseg), np.zeros((nperseg, 2))
    _lib.check(_lib.load().irrl_eval_spectrum_tables(nperseg, SPECTRUM_WINDOWS[window], float(alpha), win.ctypes.data_as(_lib.dp), tw.ctypes.data_as(_lib.dp)))
    return win, tw


def _spectrum_frames(rows, frame_first, frame_every, frames):
    frame_first, frame_every, T = _gait_frames(rows, frame_first, frame_every, frames, SPECTRUM_MAX_FRAMES)
    if T < 1:
        raise ValueError("frames lies in 1 .. %d" % SPECTRUM_MAX_FRAMES)
    return frame_first, frame_every, T


def _spectrum_tables_check(window, tw, nperseg):
    window, tw = np.asarray(window), np.asarray(tw)
    if window.shape != (nperseg,) or tw.shape != (nperseg, 2) or window.dtype != np.float64 or tw.dtype != np.float64:
        raise ValueError("window: float64 [nperseg], tw: float64 [nperseg, 2] (spectrum_tables)")
    return window, tw


def spectrum_numpy(x, rec_done, spec, window, tw, conditions=None, frame_first=0, frame_every=1, frames=None, windowed=False):
    """The twin of irrl_eval_spectrum (include/irrl_env.h): x float32 [rows, N, x_dim], rec_done [rows, N] or None, window / tw the tables of
    spectrum_tables, env = condition * robots + robot (conditions None: N, one robot each) -> dict(segments int64 [G], psd_sum float64 [G, cx, K],
    sxx float64 [M, cx, S_max, K] for the robots spec["matrix_env"] (None without any)).  Written in the stated order: per segment an explicit
    loop over n for the detrend's sum and for the DFT's two sums (every robot, column and bin at once, each as s = s + a * t from +0.0 with the
    twiddle at (k n) mod nperseg), then the power as (g_k density) (Re^2 + Im^2); the segments in ascending order from +0.0, then a condition's
    robots in ascending order from +0.0.  windowed=True: the result also carries `a` float64 [N, S_max, cx, nperseg], the detrended and windowed
    segments (0 where a robot has none), from which a test computes its bound."""
    s = spectrum_spec(**spec)
    cx, P, hop, K = s["x_count"], s["nperseg"], s["hop"], spectrum_bins(s["nperseg"])
    window, tw = _spectrum_tables_check(window, tw, P)
    x = np.asarray(x)
    if x.ndim != 3 or x.shape[2] != s["x_dim"] or x.dtype != np.float32:
        raise ValueError("x: float32 [rows, N, %d]" % s["x_dim"])
    rows, N = x.shape[:2]
    Cn, R = _motor_shape(N, N if conditions is None else conditions)
    frame_first, frame_every, T = _spectrum_frames(rows, frame_first, frame_every, frames)
    if any(e < 0 or e >= N for e in s["matrix_env"]):
        raise ValueError("a matrix_env lies outside 0 .. N - 1")
    sel = frame_first + frame_every * np.arange(T)
    te = np.full(N, T, np.int64)
    if rec_done is not None:
        done = np.asarray(rec_done)
        if done.shape != (rows, N):
            raise ValueError("rec_done [rows, N]")
        dn = done[sel] != 0
        te = np.where(dn.any(0), dn.argmax(0), T).astype(np.int64)
    S = np.where(te >= P, (te - P) // hop + 1, 0).astype(np.int64)
    S_max = (T - P) // hop + 1 if T >= P else 0
    xw = x[sel][:, :, s["x_first"]:s["x_first"] + cx]                 # float32 [T, N, cx]
    scale = np.asarray(s["scale"], np.float64)
    t = 0.0
    for n in range(P):
        t = t + window[n] * window[n]
    density = 1.0 / (s["fs"] * t)
    k = np.arange(K)
    gain = np.where((k == 0) | (2 * k == P), 1.0, 2.0)
    factor = gain * density
    part = np.zeros((N, cx, K))
    M = len(s["matrix_env"])
    sxx = np.zeros((M, cx, S_max, K)) if M else None
    a_all = np.zeros((N, S_max, cx, P)) if windowed else None
    with np.errstate(invalid="ignore", over="ignore"):
        for seg in range(int(S.max()) if N else 0):                # segments in ascending order
            on = seg < S
            v = xw[seg * hop:seg * hop + P].astype(np.float64) * scale          # [P, N, cx]
            if s["detrend"]:
                m = np.zeros((N, cx))
                for n in range(P):
                    m = m + v[n]
                m = m / float(P)
                v = v - m
            a = v * window[:, None, None]
            re, si = np.zeros((N, cx, K)), np.zeros((N, cx, K))
            j = np.zeros(K, np.int64)
            for n in range(P):                                     # samples in ascending order
                re = re + a[n][:, :, None] * tw[j, 0]
                si = si + a[n][:, :, None] * tw[j, 1]
                j = (j + k) % P
            im = -si
            p = factor * (re * re + im * im)
            part = np.where(on[:, None, None], part + p, part)
            for mi, e in enumerate(s["matrix_env"]):
                if on[e]:
                    sxx[mi, :, seg, :] = p[e]
            if windowed:
                a_all[on, seg] = np.transpose(a, (1, 2, 0))[on]
        part = part.reshape(Cn, R, cx, K)
        tot = np.zeros((Cn, cx, K))
        for r in range(R):                                         # robots in ascending order
            tot = tot + part[:, r]
    out = dict(segments=S.reshape(Cn, R).sum(1).astype(np.int64), psd_sum=tot, sxx=sxx)
    if windowed:
        out["a"] = a_all
    return out


def spectrum_struct(spec):
    from . import _lib
    s = spectrum_spec(**spec)
    st = _lib.EvalSpectrumSpec(**{k: s[k] for k in ("x_dim", "x_first", "x_count", "nperseg", "hop", "detrend")}, matrix_count=len(s["matrix_env"]), fs=s["fs"])
    for i, e in enumerate(s["matrix_env"]):
        st.matrix_env[i] = e
    for i, v in enumerate(s["scale"]):
        st.scale[i] = v
    return st


def spectrum_work(num_envs, spec):
    """the doubles of `work` for a pool of num_envs: irrl_eval_spectrum_work = num_envs * (cx K + 1)"""
    s = spectrum_spec(**spec)
    return int(num_envs) * (s["x_count"] * spectrum_bins(s["nperseg"]) + 1)


def spectrum_device(x, rec_done, spec, window, tw, conditions=None, frame_first=0, frame_every=1, frames=None, sxx=True, work="auto"):
    """spectrum_numpy on the device: ONE call of irrl_eval_spectrum on torch's current stream (one workgroup per robot and block of four columns
    and, with more than one robot per condition, a second launch that adds the robots' partials in order), no synchronisation.  x: a float32
    device tensor [rows, N, x_dim], rec_done a bool / uint8 device tensor [rows, N] or None; window, tw: the tables of spectrum_tables as numpy
    arrays (uploaded here) or float64 device tensors.  sxx=False: no spectrograms although the spec lists robots.  work: "auto" = allocated here
    where robots > 1, None = NULL (one robot per condition only), or a float64 device tensor of spectrum_work doubles.
    -> dict of device tensors segments int64 [G], psd_sum float64 [G, cx, K], sxx float64 [M, cx, S_max, K] or None"""
    import torch
    from . import _lib
    from ._lib import ptr
    s = spectrum_spec(**spec)
    if not sxx:
        s = dict(s, matrix_env=())
    cx, P, K = s["x_count"], s["nperseg"], spectrum_bins(s["nperseg"])
    if x.dim() != 3 or x.shape[2] != s["x_dim"] or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError("x: a float32 device tensor [rows, N, %d]" % s["x_dim"])
    x = _lib.contig(x)
    rows, n = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    if rec_done is not None:
        if tuple(rec_done.shape) != (rows, n) or rec_done.device != dev or rec_done.dtype not in (torch.bool, torch.uint8):
            raise ValueError("rec_done: a bool / uint8 device tensor [rows, N]")
        rec_done = _lib.contig(rec_done).view(torch.uint8)

    def table(t, shape, what):
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.array(t)).to(dev)                  # (a copy: the caller's table may be read-only)
        if tuple(t.shape) != shape or t.dtype != torch.float64 or t.device != dev:
            raise ValueError("%s: float64 %s on the device of x (spectrum_tables)" % (what, list(shape)))
        return _lib.contig(t)
    window, tw = table(window, (P,), "window"), table(tw, (P, 2), "tw")
    Cn, R = _motor_shape(n, n if conditions is None else conditions)
    frame_first, frame_every, T = _spectrum_frames(rows, frame_first, frame_every, frames)
    S_max = (T - P) // s["hop"] + 1 if T >= P else 0
    if isinstance(work, str) and work == "auto":
        work = torch.empty(spectrum_work(n, s), device=dev, dtype=torch.float64) if R > 1 else None
    elif work is not None and (work.dtype != torch.float64 or work.numel() < spectrum_work(n, s) or work.device != dev or not work.is_contiguous()):
        raise ValueError("work: a contiguous float64 device tensor of at least %d elements" % spectrum_work(n, s))
    M = len(s["matrix_env"])
    st = spectrum_struct(s if S_max > 0 else dict(s, matrix_env=()))      # (no segment anywhere: `sxx` is empty, and an empty tensor has no address)
    out = dict(segments=torch.zeros(Cn, device=dev, dtype=torch.int64), psd_sum=torch.zeros(Cn, cx, K, device=dev, dtype=torch.float64),
               sxx=torch.zeros(M, cx, S_max, K, device=dev, dtype=torch.float64) if M else None)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().irrl_eval_spectrum(ptr(x), ptr(rec_done), rows, n, Cn, R, frame_first, frame_every, T, C.cast(C.pointer(st), C.c_void_p),
                                                  ptr(window), ptr(tw), ptr(out["segments"]), ptr(out["psd_sum"]), ptr(out["sxx"]), ptr(work),
                                                  _lib.stream_ptr(dev)))
    return out


def spectrum_to_numpy(res):
    """a result of spectrum_device -> the twin's dict of numpy arrays (synchronises)"""
    return {k: None if v is None else v.cpu().numpy() for k, v in res.items()}


def spectrum_row(psd_sum, segments, fs, names, band_hz, nperseg=None):
    """One condition's Welch spectra -> per signal group `name` of names the keys vib_peak_hz_<name>, the frequency of the largest bin of the
    group's spectrum without bin 0, and vib_frac_<name>, the fraction of the group's power in the bins above band_hz (of the power in the bins
    k >= 1; the bins are equally wide, so the sums are the integrals).  psd_sum: name -> float64 [cx, K] (the call's sums of one condition),
    segments: name -> int, or one int for all; the group's spectrum is the sum over its columns of psd_sum / segments.  nperseg: the segment
    length behind the K bins (None: the even one, 2 (K - 1); an odd one has to be named).  NaN for both keys where the group has no segment or
    its power is not a positive finite number."""
    out = {}
    for name in names:
        p = np.asarray(psd_sum[name], np.float64)
        n = int(segments[name] if isinstance(segments, dict) else segments)
        K = p.shape[-1]
        P = 2 * (K - 1) if nperseg is None else int(nperseg)
        if spectrum_bins(P) != K:
            raise ValueError("spectrum_row: nperseg = %d does not have %d bins" % (P, K))
        peak = frac = float("nan")
        if n > 0:
            with np.errstate(invalid="ignore", over="ignore"):
                w = p.reshape(-1, K).sum(0) / n
                total = float(w[1:].sum())
            if math.isfinite(total) and total > 0:
                f = spectrum_frequencies(P, fs)
                peak = float(f[1 + int(np.argmax(w[1:]))])
                frac = float(w[1:][f[1:] > float(band_hz)].sum() / total)
        out["vib_peak_hz_" + name], out["vib_frac_" + name] = peak, frac
    return out


# ---- the device loop ----
def resolve_persistent(persistent, supported):
    """the `persistent` keyword of PolicyEvaluator.run / robustness_sweep (False, True, "auto"; the command line's "off" / "on" too) -> bool;
    supported: a callable, asked for "auto" only"""
    if persistent in (False, None, "off"):
        return False
    if persistent in (True, "on"):
        return True
    if persistent == "auto":
        return bool(supported())
    raise ValueError("persistent is False, True or 'auto', not %r" % (persistent,))


class PolicyEvaluator(object):
    """PolicyEvaluator(env_impl, policy, delay, cmd, cmd_hz=1.0, vel_hz=None, act_hz=None, clip=True)

    env_impl: an initialised FlexibleGymEnv (Manual mode: the evaluator owns obs[0:3]); policy: a CustomLSTMPolicy or an MlpPolicy with
    layers (64, 64) on the pool's device (the latter has no recurrent state: `lstm_state` is None, and the loop runs through the C-ABI's
    irrl_mlp_eval_measured[_persistent], the one pair of entry points that exists for it);
    delay [N] control steps and cmd [N] (v_x) or [N, 3] per env; depth: length of the delay line (default max(delay) + 1).
    Friction goes through env_impl.SetContactCoefficient between `run` calls (a warm-up on another material = two calls)."""

    def __init__(self, env_impl, policy, delay, cmd, cmd_hz=1.0, vel_hz=None, act_hz=None, clip=True, depth=None):
        import torch
        self.env, self.policy = env_impl, policy
        self.n = n = env_impl.getNumOfEnvs()
        self.dev = dev = torch.device("cuda", env_impl.device_index)
        from .policies import CustomLSTMPolicy, MlpPolicy
        self.is_mlp = isinstance(policy, MlpPolicy)
        if self.is_mlp:
            layers = tuple(int(l.w.shape[1]) for l in policy.pi_fc)
            if (layers != (64, 64) or tuple(int(l.w.shape[1]) for l in policy.vf_fc) != layers or int(policy.pi_fc[0].w.shape[0]) != 35
                    or policy.act_dim != 12):
                raise ValueError("PolicyEvaluator runs MlpPolicy with layers (64, 64), 35 observations and 12 actions")
            self.hid = 64
        elif isinstance(policy, CustomLSTMPolicy):
            self.hid = int(policy.n_lstm[0])
            if len(policy.n_lstm) != 2 or policy.n_lstm[0] != policy.n_lstm[1] or self.hid not in (32, 48, 64) or policy.act_dim != 12:
                raise ValueError("PolicyEvaluator runs CustomLSTMPolicy with two equal LSTM layers of 32, 48 or 64 units and 12 actions")
        else:
            raise ValueError("PolicyEvaluator runs CustomLSTMPolicy (two equal LSTM layers of 32, 48 or 64 units) or MlpPolicy (layers (64, 64)), "
                             "not %s" % type(policy).__name__)
        delay, self.depth = _delay_rows(delay, n, depth)
        cfg = {k: env_impl.cfg_value(k) for k in ("abad", "Vx", "Vy", "Omega", "control_dt")}
        mean, std, _, _ = obs_normalisation(cfg)
        self.cmd_mean, self.cmd_std = (C.c_float * 3)(*mean[0:3]), (C.c_float * 3)(*std[0:3])
        dt = cfg["control_dt"]
        self.a_cmd, self.a_vel, self.a_act = (float(np.float32(lowpass_alpha(dt, f))) for f in (cmd_hz, vel_hz, act_hz))
        self.clip = bool(clip)
        f32 = dict(device=dev, dtype=torch.float32)
        self.delay = torch.from_numpy(delay.astype(np.int32)).to(dev)
        self.cmd_target = torch.from_numpy(_cmd_rows(cmd, n).astype(np.float32)).to(dev)
        self.ring = torch.zeros(self.depth, n, 35, **f32)
        self.cmd = torch.zeros(n, 3, **f32)
        self.vel_his = torch.zeros(n, 35, **f32)
        self.act_his = torch.zeros(n, 12, **f32)
        self.lstm_state = None if self.is_mlp else torch.zeros(n, 8 * self.hid, **f32)     # MlpPolicy has no recurrent state
        self.done = torch.zeros(n, dtype=torch.bool, device=dev)
        self.obs = torch.zeros(n, 35, **f32)
        self.work = torch.zeros(n, WORK_DIM, **f32)
        self.stats = torch.zeros(len(STAT_SLOTS), n, device=dev, dtype=torch.float64)
        self.heading_int = torch.zeros(n, **f32)               # the heading hold's integrator I (evaluator state, like cmd)
        self._omega, self._dt = float(cfg["Omega"]), float(dt)
        # the gait measurements (set_scenario(gait=True)): f64 sums [B, 20, N] or None; the contact flags of the previous step (evaluator state)
        self.gait = None
        self.prev_contact = torch.zeros(n, 4, device=dev, dtype=torch.uint8)
        self.scenario = None
        # which C entry points `run` calls: "auto" = the narrowest list that takes what is installed (irrl_lstm_eval_rollout / _scenario /
        # _perturbed / _measured); "perturbed" = always the kick table's, "measured" = always the gait measurements', with NULL for what is not
        # installed -- the same code path by construction (the narrower entry points are calls of the wider ones with NULL), which is what the
        # tests hold them to.  MlpPolicy has the widest pair only (irrl_mlp_eval_measured[_persistent]): "auto" and "measured" are that pair
        self.entry_points = "auto"
        self.t = 0
        self.reset()

    def reset(self):
        """reset every env; the reset observation fills the delay line, command / histories / LSTM state / done / the heading integrator are
        zeroed, t = 0.  An installed scenario stays and its origin is re-based with the counter: t0 becomes what it was relative to the counter
        when the scenario was installed (installed at t = 100 with the default t0: 0 again; installed with t0 = t + 1000: 1000)"""
        self.env.reset(self.obs)
        self.ring.copy_(self.obs.unsqueeze(0).expand_as(self.ring))
        for b in (self.cmd, self.vel_his, self.act_his, self.lstm_state, self.heading_int):
            if b is not None:
                b.zero_()
        self.done.zero_()
        self.prev_contact.zero_()
        self.t = 0
        if self.scenario is not None:
            self.scenario["t0"] = self.scenario["t0_rel"]

    def set_scenario(self, cmd_schedule=None, cmd_every=1, heading=None, stat_buckets=1, stat_every=1, t0=None, kicks=None, kick_first=0, kick_every=1,
                     gait=False):
        """Install a scenario (include/irrl_env.h irrl_eval_scenario) for the following `run` calls; with tau = max(t - t0, 0):
        cmd_schedule [S, N] (v_x) or [S, N, 3]: the command target of step t is row min(tau // cmd_every, S - 1) (None: the constructor's cmd);
        heading: a dict of ref, kp, ki (a scalar or [N] each) and windup (None: the config's Omega) -- heading_hold(...) --, the PI loop on the base
        yaw whose output the actor sees as element 2, for the envs with a non-zero gain (None: off);
        stat_buckets B, stat_every: the frame of step t goes to bucket min(tau // stat_every, B - 1) of `stats`, which becomes [B, 18, N] and starts
        from zero; t0: the origin on the global step counter (default: the current self.t).  The heading integrator keeps its value.
        kicks [N, 11] or [R, N, 11] (kick_rows) with kick_first, kick_every: row r displaces the base state of the envs whose row is on at the
        start of env step t0 + kick_first + r kick_every (include/irrl_env.h irrl_eval_kicks; None: no kicks).
        gait: measure joint power, torque and ground-force sums and the footfall pattern (include/irrl_env.h irrl_eval_gait) into `gait`
        [B, 20, N] (GAIT_SLOTS), bucketed like `stats` and zeroed here; read with gait_statistics / bucket_gait_statistics."""
        import torch
        f32 = dict(device=self.dev, dtype=torch.float32)
        table = self.cmd_target.unsqueeze(0) if cmd_schedule is None else torch.from_numpy(_schedule_rows(cmd_schedule, self.n).astype(np.float32)).to(self.dev)
        cmd_every, stat_buckets, stat_every = int(cmd_every), int(stat_buckets), int(stat_every)
        if cmd_every < 1 or stat_buckets < 1 or stat_every < 1:
            raise ValueError("cmd_every, stat_buckets and stat_every are at least 1")
        h = heading_parameters(heading, self.n, self._omega, self._dt)
        t0 = int(self.t if t0 is None else t0)
        if kicks is not None:
            kick_first, kick_every = _kick_schedule(kick_first, kick_every)
            kicks = dict(table=torch.from_numpy(_kick_table(kicks, self.n)).to(self.dev), first=kick_first, every=kick_every)
        self.scenario = dict(t0=t0, t0_rel=t0 - self.t, cmd_table=table.contiguous(), cmd_every=cmd_every, stat_buckets=stat_buckets,
                             stat_every=stat_every, heading=None if h is None else dict(
                                 {k: torch.from_numpy(h[k].astype(np.float32)).to(self.dev) for k in ("ref", "kp", "ki")},
                                 windup=float(np.float32(h["windup"])), dt=float(np.float32(h["dt"]))), kicks=kicks)
        self.stats = torch.zeros(stat_buckets, len(STAT_SLOTS), self.n, device=self.dev, dtype=torch.float64)
        self.gait = torch.zeros(stat_buckets, len(GAIT_SLOTS), self.n, device=self.dev, dtype=torch.float64) if gait else None

    def clear_scenario(self):
        """back to the constructor's constant command, no heading hold, one statistics window [18, N] (zeroed)"""
        import torch
        self.scenario = None
        self.stats = torch.zeros(len(STAT_SLOTS), self.n, device=self.dev, dtype=torch.float64)
        self.gait = None

    def _scenario_struct(self):
        from ._lib import EvalScenario, ptr
        s = self.scenario
        h = s["heading"]
        raw = lambda t: None if t is None else ptr(t).value
        return EvalScenario(t0=s["t0"], cmd_rows=int(s["cmd_table"].shape[0]), cmd_every=s["cmd_every"], cmd_table=raw(s["cmd_table"]),
                            stat_buckets=s["stat_buckets"], stat_every=s["stat_every"], heading_ref=raw(h and h["ref"]), heading_kp=raw(h and h["kp"]),
                            heading_ki=raw(h and h["ki"]), heading_int=raw(self.heading_int), heading_windup=h["windup"] if h else 0.0,
                            heading_dt=h["dt"] if h else 0.0)

    def _kicks_struct(self):
        from ._lib import EvalKicks, ptr
        k = self.scenario["kicks"]
        return EvalKicks(kick_rows=int(k["table"].shape[0]), kick_first=k["first"], kick_every=k["every"], kick_table=ptr(k["table"]).value)

    def perturb_base(self, rows):
        """displace the pool's robots now, one kick row per env (the module's perturb_base)"""
        perturb_base(self.env, rows)

    @property
    def persistent_supported(self):
        """does the persistent single-launch kernel exist for this pool and policy (16-lane layout, kernel variant shipped_flat / shipped / md;
        CustomLSTMPolicy of 48 units or MlpPolicy)?"""
        from . import _lib
        lib = _lib.load()
        rc = (lib.irrl_mlp_eval_rollout_supports if self.is_mlp else lib.irrl_lstm_eval_rollout_supports)(self.env._h, self.hid)
        if rc < 0:
            raise RuntimeError(_lib.last_error())
        return rc == 1

    @property
    def auto_persistent(self):
        """what persistent="auto" resolves to: the persistent launch where it exists and is the measured-faster form.  For CustomLSTMPolicy that
        is wherever it exists; for MlpPolicy see mlp_auto_persistent."""
        if not self.persistent_supported:
            return False
        return mlp_auto_persistent(self.n) if self.is_mlp else True

    def run(self, steps, record=(), accumulate=True, persistent=False):
        """`steps` control steps from ONE C call (stream-ordered on torch's current stream, no synchronisation).  record: names out of
        RECORDERS, and "gait" (rec_gait [steps, N, 32]: tq | qd | in_contact | lam_w_z / control_dt) -> dict of device tensors [steps, N, .]; accumulate: add these steps' frames to the per-env statistics.
        The trace recorders "lstm" ([steps, N, 4 hid]: the actor's half of the recurrent state, c0 | h0 | c1 | h1, AFTER each step's policy step;
        steps x N x 4 hid x 4 B) and "value" ([steps, N]: the critic's value of each step) exist in the five-launch form only (include/irrl_env.h
        irrl_eval_trace: one extra launch per step, every other buffer bit-identical): with one of them persistent=True raises ValueError and
        "auto" is the five-launch form; "lstm" with an MlpPolicy raises ValueError, the policy has no recurrent state.
        persistent: False = five launches per control step (every pool and policy; also steps the critic's half of lstm_state); True = the
        whole call as one persistent launch (raises with the library's text where the kernel does not exist); "auto" = the persistent launch
        where `persistent_supported`, else five launches per step.  The two forms leave bit-identical buffers -- except the critic's half of
        lstm_state and the `value` column of the work array, which the persistent form does not touch -- and may follow each other.
        With an MlpPolicy both forms run both networks and every buffer is bit-identical, the whole work array included; "auto" is
        resolved by `auto_persistent`."""
        import torch
        from . import _lib
        from ._lib import ptr
        from .lstm_fused import _head_ptrs, _lstm_weight_table, _mlp_weight_table
        steps = int(steps)
        unknown = [k for k in record if k not in RECORDERS and k != "gait" and k not in TRACE_RECORDERS]
        if unknown:
            raise KeyError("unknown recorder(s) %s: choose from %s" % (unknown, sorted(RECORDERS) + ["gait"] + list(TRACE_RECORDERS)))
        trace = [k for k in TRACE_RECORDERS if k in record]
        if "lstm" in trace and self.is_mlp:
            raise ValueError("the recorder 'lstm' needs a recurrent policy: MlpPolicy has no recurrent state")
        if trace and persistent in (True, "on"):
            raise ValueError("the trace recorder(s) %s exist in the five-launch form only: the persistent kernel keeps the recurrent state in an LDS "
                             "allocation that is full (163 264 of 163 840 B) and does not run the critic -- use persistent=False or 'auto'" % trace)
        out = {}
        for k in record:
            shape = (steps, self.n) + ((4 * self.hid,) if k == "lstm" else () if k == "value" else (GAIT_REC_DIM,) if k == "gait"
                                       else (RECORDERS[k],) if RECORDERS[k] else ())
            out[k] = torch.empty(shape, device=self.dev, dtype=torch.bool if k == "done" else torch.float32)
        with torch.cuda.device(self.dev):
            if self.is_mlp:
                warr = _mlp_weight_table(self.policy)
            else:
                self.policy.prepare()                          # the kernels' permuted weight copies follow the parameters (a learner may have stepped)
                warr = _lstm_weight_table(self.policy, self.dev)
            lib = _lib.load()
            one_launch = resolve_persistent(persistent, lambda: self.auto_persistent) and not trace
            if self.is_mlp and self.entry_points not in ("auto", "measured"):
                raise ValueError("entry_points is 'auto' or 'measured' for an MlpPolicy (only the widest pair of entry points exists for it)")
            if self.entry_points not in ("auto", "perturbed", "measured"):
                raise ValueError("entry_points is 'auto', 'perturbed' or 'measured'")
            has_kicks = self.scenario is not None and self.scenario["kicks"] is not None
            struct = None if self.scenario is None else self._scenario_struct()
            kstruct = self._kicks_struct() if has_kicks else None
            raw = lambda st: None if st is None else C.cast(C.pointer(st), C.c_void_p)
            # the gait measurements: the sums where installed and accumulating, the recorder where asked for; with the sums installed prev_contact
            # goes along through unmeasured steps too (a warm-up), so that the first measured step knows its predecessor's flags
            gstruct = None
            if self.gait is not None or "gait" in out:
                gstruct = _lib.EvalGait(gait=ptr(self.gait).value if (self.gait is not None and accumulate) else None,
                                        prev_contact=ptr(self.prev_contact).value if self.gait is not None else None,
                                        rec_gait=ptr(out["gait"]).value if "gait" in out else None)
            if trace:                                          # the widest list with the trace struct behind the gait measurements'
                tstruct = _lib.EvalTrace(rec_lstm=ptr(out["lstm"]).value if "lstm" in out else None,
                                         rec_value=ptr(out["value"]).value if "value" in out else None)
                fn = lib.irrl_mlp_eval_traced if self.is_mlp else lib.irrl_lstm_eval_traced
                scenario = (raw(struct), raw(kstruct), raw(gstruct), raw(tstruct))
            elif self.is_mlp:
                fn = lib.irrl_mlp_eval_measured_persistent if one_launch else lib.irrl_mlp_eval_measured
                scenario = (raw(struct), raw(kstruct), raw(gstruct))
            elif gstruct is not None or self.entry_points == "measured":
                fn = lib.irrl_lstm_eval_measured_persistent if one_launch else lib.irrl_lstm_eval_measured
                scenario = (raw(struct), raw(kstruct), raw(gstruct))
            elif has_kicks or self.entry_points == "perturbed":  # the kick table's struct behind the scenario's
                fn, scenario = (lib.irrl_lstm_eval_perturbed_persistent if one_launch else lib.irrl_lstm_eval_perturbed), (raw(struct), raw(kstruct))
            elif self.scenario is not None:                    # the scenario entry points: the same list with the host struct in front of the stream
                fn, scenario = (lib.irrl_lstm_eval_scenario_persistent if one_launch else lib.irrl_lstm_eval_scenario), (raw(struct),)
            else:
                fn, scenario = (lib.irrl_lstm_eval_rollout_persistent if one_launch else lib.irrl_lstm_eval_rollout), ()
            _lib.check(fn(
                self.env._h, steps, self.t, self.hid, 35, 12, warr, *_head_ptrs(self.policy), self.depth, ptr(self.ring), ptr(self.cmd), ptr(self.vel_his),
                ptr(self.act_his), *(() if self.is_mlp else (ptr(self.lstm_state),)), ptr(self.done), ptr(self.obs), ptr(self.work), ptr(self.delay), ptr(self.cmd_target),
                self.a_cmd, self.a_vel, self.a_act, self.cmd_mean, self.cmd_std, int(self.clip), *[ptr(out.get(k)) for k in RECORDERS],
                ptr(self.stats) if accumulate else None, *scenario, _lib.stream_ptr(self.dev)))
        self.t += steps
        return out

    def zero_statistics(self):
        self.stats.zero_()
        if self.gait is not None:
            self.gait.zero_()

    def measure_gait(self, on=True):
        """switch the gait measurements on (zeroed sums, one bucket per statistics bucket) or off without touching the scenario; set_scenario(...,
        gait=True) is this behind the scenario's installation"""
        import torch
        buckets = self.stats.shape[0] if self.stats.dim() == 3 else 1
        self.gait = torch.zeros(buckets, len(GAIT_SLOTS), self.n, device=self.dev, dtype=torch.float64) if on else None

    def total_mass(self):
        """per-env total mass [N] (trunk + 12 links, IRRL_S_MASS of get_state: randomised per env under StochasticDynamics)"""
        return np.asarray(self.env.get_state(), np.float64)[:, _S_MASS:_S_MASS + 13].sum(1)

    def _gait_sums(self):
        if self.gait is None:
            raise RuntimeError("no gait measurements installed: set_scenario(..., gait=True)")
        sums, body = self.gait.cpu().numpy(), self.stats.cpu().numpy()
        return sums, body if body.ndim == 3 else body[None]

    def gait_statistics(self, mass=None, g=9.81):
        """power, cost of transport and footfall statistics per env over the frames accumulated since zero_statistics() (synchronises): dict of [N]
        numpy arrays, see gait_from_sums; mass: None = total_mass()"""
        sums, body = self._gait_sums()
        return gait_from_sums(gait_merge(sums), body.sum(0), self.total_mass() if mass is None else mass, self._dt, g)

    def bucket_gait_statistics(self, mass=None, g=9.81):
        """the same per bucket of the installed scenario: dict of [B, N] numpy arrays"""
        sums, body = self._gait_sums()
        mass = self.total_mass() if mass is None else mass
        per = [gait_from_sums(s, b, mass, self._dt, g) for s, b in zip(sums, body)]
        return {k: np.stack([p[k] for p in per], 0) for k in per[0]}

    def statistics(self):
        """per-env statistics over the frames accumulated since zero_statistics() (synchronises): dict of [N] numpy arrays, see statistics_from_sums"""
        sums = self.stats.cpu().numpy()
        return statistics_from_sums(sums.sum(0) if sums.ndim == 3 else sums)   # a scenario's buckets: the whole window, from the sums added

    def bucket_statistics(self):
        """the statistics per bucket of the installed scenario (synchronises): dict of [B, N] numpy arrays (B = 1 without a scenario)"""
        sums = self.stats.cpu().numpy()
        per = [statistics_from_sums(s) for s in (sums if sums.ndim == 3 else sums[None])]
        return {k: np.stack([p[k] for p in per], 0) for k in per[0]}


def load_policy(model_or_policy, device):
    """a CustomLSTMPolicy or an MlpPolicy on `device` from: the policy itself, a model that has `.policy` (PPO2), the path of a checkpoint (this
    build's or a stable-baselines pickle of the reference; which of the two policies it holds is decided from the shapes of its tensor list,
    through MlpPolicy.sb_parameters()), or the path of an actor export `actor_*.npz` (tools/export_actor_fixture.py: two LSTM layers and the action
    head, keys wx0 ...; or MlpPolicy's actor, keys pi_w1, pi_b1, pi_w2, pi_b2, pi_w, pi_b; the critic, which the evaluation's records do not
    depend on, keeps the initialisation of torch.manual_seed(3))"""
    import torch
    from .policies import CustomLSTMPolicy, MlpPolicy
    pol = getattr(model_or_policy, "policy", model_or_policy)
    if isinstance(pol, str):
        if pol.endswith(".npz"):
            z = np.load(pol)
            torch.manual_seed(3)
            if "pi_w1" in z.files:
                pol = MlpPolicy(ob_dim=z["pi_w1"].shape[0], act_dim=z["pi_w"].shape[1], layers=(z["pi_w1"].shape[1], z["pi_w2"].shape[1]))
                ps = [p for l in pol.pi_fc for p in (l.w, l.b)] + [pol.pi.w, pol.pi.b]
                params = [z[k] for k in ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_w", "pi_b")]
            else:
                pol = CustomLSTMPolicy(ob_dim=z["wx0"].shape[0], act_dim=z["pi_w"].shape[1], n_lstm=(z["wh0"].shape[0], z["wh1"].shape[0]))
                ps = [p for l in pol.lstm_pi for p in (l.wx, l.wh, l.b)] + [pol.pi.w, pol.pi.b]
                params = [z[k] for k in ("wx0", "wh0", "b0", "wx1", "wh1", "b1", "pi_w", "pi_b")]
        else:
            from .checkpoint import mlp_checkpoint_layers, read_checkpoint
            _, params = read_checkpoint(pol)
            layers = mlp_checkpoint_layers(params)
            if layers is not None:
                ob_dim, act_dim, layers = layers
                pol = MlpPolicy(ob_dim=ob_dim, act_dim=act_dim, layers=layers)
                ps = pol.sb_parameters()
            else:
                pol = CustomLSTMPolicy(ob_dim=params[0].shape[0], act_dim=params[14].shape[1], n_lstm=(params[1].shape[0], params[4].shape[0]))
                ps = pol.sb_parameters()
                if len(ps) != len(params):
                    raise ValueError("checkpoint holds %d tensors, CustomLSTMPolicy has %d" % (len(params), len(ps)))
        with torch.no_grad():
            for p, a in zip(ps, params):
                p.copy_(torch.as_tensor(np.asarray(a), dtype=p.dtype).reshape(p.shape))
    pol = pol.to(device)
    if hasattr(pol, "prepare"):
        pol.prepare()
    return pol


def robustness_sweep(model_or_policy, env_cfg, mus, delays, cmds, warm_steps=1000, steps=2000, cmd_hz=1.0, vel_hz=None, act_hz=None, clip=True,
                     mu_warm=0.8, device=None, persistent=PERSISTENT_DEFAULT, levels=None, level_steps=None, heading=None, gait=False,
                     mass=None, g=9.81, recurrence=None, recurrence_frames=None, record_body=False, footfall=None, motor=None, record_gait=False,
                     correlation=None, record_correlation=False, spectrum=None, record_spectrum=False):
    """The reference's robustness grid in one pool: len(mus) x len(delays) x len(cmds) Manual-mode envs (condition index = (i_mu * len(delays) +
    i_delay) * len(cmds) + i_cmd), `warm_steps` control steps on friction mu_warm, then `steps` on the condition's own friction over which the
    statistics are taken.  env_cfg: the `environment:` mapping of a config.  persistent: PolicyEvaluator.run's keyword (same statistics bit for bit
    either way).  -> list of rows dict(mu, delay, cmd, falls, frames, <statistics>).
    heading: a heading_hold dict (a scalar or one value per condition), the script's `--dir_fd`, on from the first step.
    levels (with an even level_steps): the script's `--step` staircase in place of `steps` at the full command -- level l = 1 .. levels commands
    l / levels * cmd for level_steps control steps (the warm-up runs at level 1), the run is levels * level_steps steps, still ONE call, with two
    statistics buckets per level; -> one row per (condition, level), taken over the SECOND half of the level, with the keys `level` and
    `cmd_level` (the commanded v_x of that level).
    gait: every row gains the keys of gait_from_sums over the same frames -- cot, power_mean, duty0 .. 3, stride_hz0 .. 3, ... -- with `mass`
    (None: each env's own total) and g; off, the rows are what they were.
    recurrence: a spec (RECURRENCE_SPEC_REFERENCE) -- the body recorder is kept on the device for the run and every row gains `recurrence` =
    dict(RR, DET, L, LMAX, LAM, TT, period_s, period_fraction, kept) (recurrence_row: the measures of irrl_eval_recurrence and the stride period
    out of the lag words 0 .. T / 2 from the Theiler window on) over the LAST recurrence_frames = T frames of the run (default: min(steps, 800));
    with a staircase over the last T frames of each level's second half (refused if they do not fit); the rows of the first 8 conditions also
    carry `matrix` uint8 [T, T], the levels of the recurrence plot.  record_body: every row carries `body` [steps, 13] (staircase: [level_steps,
    13], the level's frames), whose last T frames the recurrence analysis saw.
    footfall: a spec (FOOTFALL_SPEC_REFERENCE) / motor: a spec (motor_spec(env_cfg)) -- the gait recorder and the `done` recorder are kept on the
    device for the run and every row gains `footfall` (footfall_row: debounced duty, stride period and frequency, stance and swing times, flight,
    the legs' phase lags, the gait's name; plus `counts` [4, 14], `support` [16], `phase` [3, bins]) and / or `motor` (motor_plane_row: the
    saturated, outside, motoring and braking fractions per joint; plus `counts` [12, 6], `fold` [period, 3]) over the frames the row's statistics
    cover (staircase: the second half of the level); the rows of the first 8 conditions also carry `pattern` uint8 [frames] (the gait diagram)
    and `hist` uint32 [12, t_bins, w_bins].  record_gait: every row carries `rec_gait` [frames, 32] and `rec_done` [frames], the words the two
    analyses saw.
    correlation: dict(x="contact", y="lstm"), two names out of CORR_SOURCES -- the reference's `--corr`: the recorders of the two sources (and
    `done`) are kept on the device for the MEASURED steps only (the warm-up records nothing; the LSTM state's recorder is steps x N x 4 hid x 4 B,
    1000 steps x 4096 robots x 192 units = 3.1 GB) in the five-launch form of the loop (`persistent` must not be True), irrl_eval_correlation runs
    per robot over the frames the row's statistics cover, and every row gains `corr_max` (the largest |r| of a pair, NaN if no pair has an r),
    `corr_r` (that r), `corr_leg` (its x column: the leg's name for "contact") and `corr_unit` (its y column: (layer, "c" or "h", index) for
    "lstm") -- correlation_row; the rows of the first 8 conditions also carry `corr` float64 [cx, cy], the matrix r, and `corr_moments`, the
    condition's sums.  record_correlation: every row carries `corr_x` [frames, cx], `corr_y` [frames, cy] and `rec_done` [frames], the words
    the analysis saw.  With an MlpPolicy the source "lstm" is refused: the policy has no recurrent state.
    spectrum: dict(nperseg=256, hop=224, window="tukey", alpha=0.25, detrend=1, band_hz=50.0, sources=("joint", "joint_rate", "action")), every
    key optional (SPECTRUM_REFERENCE, all of SPECTRUM_SOURCES) -- the reference's `--virba`: the `obs_cond`, `act_applied` and `done` recorders
    are kept on the device for the measured steps (either form of the loop, both policy kinds; no new recorder), irrl_eval_spectrum runs per
    source and robot over the frames the row's statistics cover, scaled by the observation's / action's standard deviations (rad, rad/s, rad),
    at fs = 1 / control_dt, and every row gains vib_peak_hz_<source> and vib_frac_<source> (spectrum_row) and `spectrum` = dict(freqs [K],
    segments, <source>: psd_sum [12, K]) -- the Welch spectrum is psd_sum / segments; the rows of the first 8 conditions also carry `sxx` =
    dict(<source>: [12, S_max, K]), the spectrograms.  record_spectrum: every row carries `spec_x` = dict(<source>: [frames, 12] float32) and
    `rec_done` [frames], the words the analysis saw.
    Without these keywords the rows are what they were, key for key."""
    import torch
    import yaml
    from . import __BLACKPANTHER_V55_RESOURCE_DIRECTORY__ as rsc
    from .flexible_robot import FlexibleGymEnv
    grid = [(float(m), int(d), float(c)) for m in mus for d in delays for c in cmds]
    if not grid:
        raise ValueError("empty sweep")
    if recurrence is not None:
        recurrence = recurrence_spec(recurrence)
        window = (int(level_steps) // 2 if level_steps is not None else 0) if levels is not None else int(steps)
        T_rec = min(window, 800) if recurrence_frames is None else int(recurrence_frames)
        if T_rec < 1 or T_rec > RECURRENCE_MAX_FRAMES:
            raise ValueError("recurrence_frames lies in 1 .. %d" % RECURRENCE_MAX_FRAMES)
        if T_rec > window:
            raise ValueError("recurrence_frames = %d does not fit %s" % (T_rec, "the second half of a level" if levels is not None else "the run's steps"))
    elif recurrence_frames is not None:
        raise ValueError("recurrence_frames needs a recurrence spec")
    cfg = dict(env_cfg.get("environment", env_cfg))
    cfg["num_envs"] = len(grid)
    cfg["Manual"] = True
    dev_index = torch.cuda.current_device() if device is None else int(device)
    env = FlexibleGymEnv(rsc, yaml.safe_dump(cfg, default_flow_style=False, width=float("inf")), device=dev_index)
    env.init()
    policy = load_policy(model_or_policy, torch.device("cuda", dev_index))
    coeff = contact_material([mu_warm if warm_steps > 0 else g[0] for g in grid])
    env.SetContactCoefficient(coeff)
    ev = PolicyEvaluator(env, policy, [g[1] for g in grid], [g[2] for g in grid], cmd_hz=cmd_hz, vel_hz=vel_hz, act_hz=act_hz, clip=clip)
    if levels is not None:
        levels = int(levels)
        if levels < 1 or level_steps is None or int(level_steps) < 2 or int(level_steps) % 2:
            raise ValueError("a staircase needs levels >= 1 and an even level_steps >= 2")
        level_steps = int(level_steps)
        steps = levels * level_steps
        # the origin behind the warm-up: tau = 0 until then, so the warm-up runs at level 1 (and with the heading hold on)
        ev.set_scenario(cmd_schedule=staircase_schedule([g[2] for g in grid], levels), cmd_every=level_steps, heading=heading, stat_buckets=2 * levels,
                        stat_every=level_steps // 2, t0=max(int(warm_steps), 0), gait=gait)
    elif heading is not None or gait:
        ev.set_scenario(heading=heading, gait=gait)
    if warm_steps > 0:
        ev.run(warm_steps, accumulate=False, persistent=persistent)
        coeff[:, 0] = [g[0] for g in grid]                     # (the setter's copy is ordered on the pool's stream, behind the warm-up)
        env.SetContactCoefficient(coeff)
    ev.zero_statistics()
    want_gait = footfall is not None or motor is not None or record_gait
    if footfall is not None:
        footfall = footfall_spec(footfall)
    if motor is not None:
        motor = motor_spec_check(motor)
    corr = None
    if correlation is not None:
        names = (correlation.get("x", "contact"), correlation.get("y", "lstm"))
        if ev.is_mlp and "lstm" in names:
            raise ValueError("correlation with the source 'lstm': the policy is an MlpPolicy and has no recurrent state (choose another source, e.g. "
                             "'action' or 'value')")
        srcs = [correlation_source(k, None if ev.is_mlp else ev.hid) for k in names]
        corr = dict(names=names, recs=[s[0] for s in srcs],
                    spec=correlation_spec(srcs[0][1], srcs[0][2], srcs[0][3], srcs[1][1], srcs[1][2], srcs[1][3]))
    elif record_correlation:
        raise ValueError("record_correlation needs correlation=dict(x=..., y=...)")
    vib = None
    if spectrum is not None:
        unknown = set(spectrum) - set(SPECTRUM_REFERENCE) - {"sources"}
        if unknown:
            raise ValueError("spectrum: unknown keys %s" % sorted(unknown))
        vib = dict(SPECTRUM_REFERENCE, sources=tuple(SPECTRUM_SOURCES))
        vib.update(spectrum)
        vib["sources"] = tuple(vib["sources"])
        for k in vib["sources"]:
            if k not in SPECTRUM_SOURCES:
                raise KeyError("unknown spectrum source %r: choose from %s" % (k, sorted(SPECTRUM_SOURCES)))
        _, obs_std, _, act_std = obs_normalisation({k: env.cfg_value(k) for k in ("abad", "Vx", "Vy", "Omega")})
        listed = tuple(range(min(len(grid), SPECTRUM_MAX_MATRICES)))
        vib["specs"] = {}
        for k in vib["sources"]:
            rec_name, c0, cn = SPECTRUM_SOURCES[k]
            std = obs_std if rec_name == "obs_cond" else act_std
            vib["specs"][k] = spectrum_spec(RECORDERS[rec_name], c0, cn, vib["nperseg"], vib["hop"], 1.0 / ev._dt, scale=std[c0:c0 + cn],
                                            detrend=vib["detrend"], matrix_env=listed)
        vib["tables"] = spectrum_tables(vib["nperseg"], vib["window"], vib["alpha"])
    elif record_spectrum:
        raise ValueError("record_spectrum needs spectrum=dict(...)")
    if recurrence is None and not record_body and not want_gait and corr is None and vib is None:
        ev.run(steps, persistent=persistent)
        extra = lambda i, l: {}
    else:
        wanted = (("body",) if recurrence is not None or record_body else ()) + (("gait", "done") if want_gait else ())
        if corr is not None:
            wanted += tuple(corr["recs"]) + ("done",)
        if vib is not None:
            wanted += tuple(SPECTRUM_SOURCES[k][0] for k in vib["sources"]) + ("done",)
        rec = ev.run(steps, record=tuple(dict.fromkeys(wanted)), persistent=persistent)              # (each recorder once, in the order asked for)
        span = steps if levels is None else level_steps               # a row's frames: the run, or its level
        parts = []
        fparts, mparts, grec = [], [], None
        first = lambda l: 0 if levels is None else l * span + span // 2      # the frames a row's statistics cover
        count = steps if levels is None else span // 2
        if count > FOOTFALL_MAX_FRAMES and (footfall is not None or motor is not None):
            raise ValueError("footfall / motor: a row covers %d frames, more than %d" % (count, FOOTFALL_MAX_FRAMES))
        for l in range(1 if levels is None else levels):
            if footfall is not None:
                fparts.append(footfall_to_numpy(footfall_device(rec["gait"], rec["done"], footfall, frame_first=first(l), frames=count)))
            if motor is not None:
                mparts.append(motor_plane_to_numpy(motor_plane_device(rec["gait"], rec["done"], motor, frame_first=first(l), frames=count)))
        if record_gait:
            grec = (rec["gait"].cpu().numpy(), rec["done"].cpu().numpy())
        cparts, crec = [], None
        if corr is not None:
            if count > CORR_MAX_FRAMES:
                raise ValueError("correlation: a row covers %d frames, more than %d" % (count, CORR_MAX_FRAMES))
            xr, yr = rec[corr["recs"][0]], rec[corr["recs"][1]]
            for l in range(1 if levels is None else levels):
                cparts.append(correlation_to_numpy(correlation_device(xr, yr, rec["done"], corr["spec"], frame_first=first(l), frames=count)))
            if record_correlation:
                sp = corr["spec"]
                win = lambda t, a, n: (t if t.dim() == 3 else t.unsqueeze(2))[:, :, a:a + n].cpu().numpy()
                crec = (win(xr, sp["x_first"], sp["x_count"]), win(yr, sp["y_first"], sp["y_count"]), rec["done"].cpu().numpy())
        vparts, vrec = [], None
        if vib is not None:
            if count > SPECTRUM_MAX_FRAMES:
                raise ValueError("spectrum: a row covers %d frames, more than %d" % (count, SPECTRUM_MAX_FRAMES))
            tabs = [torch.from_numpy(t).to(rec["done"].device) for t in vib["tables"]]
            for l in range(1 if levels is None else levels):
                vparts.append({k: spectrum_to_numpy(spectrum_device(rec[SPECTRUM_SOURCES[k][0]], rec["done"], vib["specs"][k], tabs[0], tabs[1],
                                                                    frame_first=first(l), frames=count)) for k in vib["sources"]})
            if record_spectrum:
                vrec = ({k: rec[SPECTRUM_SOURCES[k][0]][:, :, SPECTRUM_SOURCES[k][1]:SPECTRUM_SOURCES[k][1] + SPECTRUM_SOURCES[k][2]].cpu().numpy()
                         for k in vib["sources"]}, rec["done"].cpu().numpy())
        if recurrence is not None:
            shown = list(range(min(len(grid), RECURRENCE_MAX_MATRICES)))
            for l in range(1 if levels is None else levels):
                parts.append(recurrence_to_numpy(recurrence_device(rec["body"], recurrence, frame_first=(l + 1) * span - T_rec, frames=T_rec, lags=T_rec // 2 + 1,
                                                                   matrix_env=shown)))
        body = rec["body"].cpu().numpy() if record_body else None
        rec = None

        def extra(i, l):
            out = {}
            if fparts:
                f = fparts[l]
                out["footfall"] = dict(footfall_row(f["counts"][i], f["support"][i], None if f["phase"] is None else f["phase"][i], ev._dt),
                                       counts=f["counts"][i], support=f["support"][i], phase=None if f["phase"] is None else f["phase"][i])
                if i < FOOTFALL_PATTERNS:
                    out["pattern"] = f["pattern"][:, i]
            if mparts:
                m = mparts[l]
                out["motor"] = dict(motor_plane_row(m["counts"][i]), counts=m["counts"][i], fold=None if m["fold"] is None else m["fold"][i])
                if i < FOOTFALL_PATTERNS and m["hist"] is not None:
                    out["hist"] = m["hist"][i]
            if cparts:
                out.update(correlation_row(cparts[l], corr["names"], g=i))
                if i < CORR_MATRICES:
                    one = {k: None if v is None else v[i:i + 1] for k, v in cparts[l].items()}
                    out["corr"], out["corr_moments"] = correlation_from_moments(one)["r"][0], {k: v[0] for k, v in one.items()}
            if crec is not None:
                lo = first(l)
                out["corr_x"], out["corr_y"], out["rec_done"] = crec[0][lo:lo + count, i], crec[1][lo:lo + count, i], crec[2][lo:lo + count, i]
            if vparts:
                v = vparts[l]
                out.update(spectrum_row({k: v[k]["psd_sum"][i] for k in v}, {k: int(v[k]["segments"][i]) for k in v}, 1.0 / ev._dt, vib["sources"],
                                        vib["band_hz"], nperseg=vib["nperseg"]))
                out["spectrum"] = dict({k: v[k]["psd_sum"][i] for k in v}, freqs=spectrum_frequencies(vib["nperseg"], 1.0 / ev._dt),
                                       segments=int(v[vib["sources"][0]]["segments"][i]))
                if i < SPECTRUM_MAX_MATRICES and v[vib["sources"][0]]["sxx"] is not None:
                    out["sxx"] = {k: v[k]["sxx"][i] for k in v}
            if vrec is not None:
                lo = first(l)
                out["spec_x"], out["rec_done"] = {k: a[lo:lo + count, i] for k, a in vrec[0].items()}, vrec[1][lo:lo + count, i]
            if grec is not None:
                out["rec_gait"], out["rec_done"] = grec[0][first(l):first(l) + count, i], grec[1][first(l):first(l) + count, i]
            if parts:
                out["recurrence"] = recurrence_row(parts[l]["counts"][i], parts[l]["lag"][i], T_rec, recurrence, ev._dt)
                if i < len(shown):
                    out["matrix"] = parts[l]["matrix"][i]
            if body is not None:
                out["body"] = body[l * span:(l + 1) * span, i]
            return out
    number = lambda k, x: int(x) if k in ("falls", "frames", "gait_frames") else float(x)
    if levels is None:
        st = ev.statistics()
        if gait:
            st.update(ev.gait_statistics(mass, g))
        return [dict(mu=m, delay=d, cmd=c, **{k: number(k, v[i]) for k, v in st.items()}, **extra(i, 0)) for i, (m, d, c) in enumerate(grid)]
    st = ev.bucket_statistics()
    if gait:
        st.update(ev.bucket_gait_statistics(mass, g))
    return [dict(mu=m, delay=d, cmd=c, level=l + 1, cmd_level=(l + 1) / levels * c, **{k: number(k, v[2 * l + 1, i]) for k, v in st.items()}, **extra(i, l))
            for i, (m, d, c) in enumerate(grid) for l in range(levels)]


def perturbation_study(model_or_policy, env_cfg, mus, delays, cmd, explorations, noise, warm_steps=1000, frames=1000, seed=0, record_body=False,
                       persistent=PERSISTENT_DEFAULT, bucket_steps=None, cmd_hz=1.0, vel_hz=None, act_hz=None, clip=True, mu_warm=0.8, device=None, kicks=None,
                       gait=False, mass=None, g=9.81, recurrence=None, recurrence_frames=None, ensemble=None, frame_chunk=None, ensemble_survivors=False):
    """The reference's perturbation exploration (Exp_Raw_Data/Param-*.txt: NoE explorations of FoE control steps from a base state displaced by
    z_noise, roll_noise, pitch_noise and the *_dot_noise amplitudes, per friction and observation delay) in ONE Manual-mode pool of
    len(mus) x len(delays) x explorations envs, env index = (i_mu * len(delays) + i_delay) * explorations + i_exploration, command `cmd` (v_x).
    `warm_steps` control steps on friction mu_warm (None: the condition's own from the start), then the condition's friction and ONE kick of every
    robot (exploration_kicks(N, noise, default_rng(seed)), or the given kicks [N, 11]) at the start of step warm_steps, then `frames` steps.
    Statistics buckets of bucket_steps control steps (default: frames; warm_steps >= bucket_steps): bucket 0 is the window in front of the kick,
    buckets 1 .. follow it.  persistent: PolicyEvaluator.run's keyword.
    -> list of one dict per (mu, delay): mu, delay, cmd, explorations, surviving (the fraction of explorations without a fall in the post-kick
    buckets), falls [E] (post-kick), stats (dict of [B, E] arrays, bucket_statistics), kicks [E, 11] and, with record_body, body [frames, E, 13]
    (the post-kick frames; the reference's figure scripts reshape theirs as [env, frame, exploration, ...]).
    gait: every row gains `gait`, a dict of [B, E] arrays with the keys of gait_from_sums per bucket (mass None: each env's own total).
    ensemble: a spec (ENSEMBLE_SPEC_REFERENCE) -- every row gains `ensemble`, the dict of ensemble_row per post-kick frame (t, entropy, kept,
    occupied, largest, hist, mean, std), analysed on the device from the body recorder (irrl_eval_ensemble), which is recorded for that whether or
    not record_body hands it out.  frame_chunk K: the post-kick frames run as successive calls of at most K steps (the evaluator resumes bit
    for bit), each call's recorder is analysed (and copied out with record_body) and released before the next call takes its place, so the
    device memory of the recorder is K, not `frames`, rows.  ensemble_survivors: analyse only the explorations without a post-kick fall (the
    mask is known after the last frame, so the whole recorder is kept: refused together with frame_chunk).
    ensemble None (the default): the return value is what it was, key for key.
    recurrence: a spec (RECURRENCE_SPEC_REFERENCE) -- every row gains `recurrence`, a dict of [E] arrays RR, DET, L, LMAX, LAM, TT, period_s,
    period_fraction, kept (recurrence_measures / recurrence_period per exploration, irrl_eval_recurrence on the device) over the last
    recurrence_frames = T post-kick frames (default: min(frames, 800)); it needs the whole run's recorder: refused together with frame_chunk."""
    import torch
    import yaml
    from . import __BLACKPANTHER_V55_RESOURCE_DIRECTORY__ as rsc
    from .flexible_robot import FlexibleGymEnv
    if ensemble is not None:
        ensemble = ensemble_spec(ensemble)
    elif ensemble_survivors:
        raise ValueError("ensemble_survivors needs an ensemble spec")
    if frame_chunk is not None:
        frame_chunk = int(frame_chunk)
        if frame_chunk < 1:
            raise ValueError("frame_chunk >= 1")
        if ensemble_survivors:
            raise ValueError("ensemble_survivors needs the whole run's recorder: it does not go with frame_chunk")
    conditions = [(float(m), int(d)) for m in mus for d in delays]
    E, warm_steps, frames = int(explorations), int(warm_steps), int(frames)
    if recurrence is not None:
        recurrence = recurrence_spec(recurrence)
        if frame_chunk is not None:
            raise ValueError("recurrence needs the whole run's recorder: it does not go with frame_chunk")
        T_rec = min(frames, 800) if recurrence_frames is None else int(recurrence_frames)
        if T_rec < 1 or T_rec > min(frames, RECURRENCE_MAX_FRAMES):
            raise ValueError("recurrence_frames lies in 1 .. min(frames, %d)" % RECURRENCE_MAX_FRAMES)
    elif recurrence_frames is not None:
        raise ValueError("recurrence_frames needs a recurrence spec")
    bucket_steps = frames if bucket_steps is None else int(bucket_steps)
    if not conditions or E < 1 or frames < 1:
        raise ValueError("empty study")
    if bucket_steps < 1 or warm_steps < bucket_steps:
        raise ValueError("1 <= bucket_steps <= warm_steps: bucket 0 is the window in front of the kick")
    n = len(conditions) * E
    if ensemble is not None:
        _ensemble_shape(n, len(conditions))                    # (refused here, in front of the pool's allocation)
    kicks = exploration_kicks(n, noise, np.random.default_rng(seed)) if kicks is None else _kick_table(kicks, n)[0]
    cfg = dict(env_cfg.get("environment", env_cfg))
    cfg["num_envs"] = n
    cfg["Manual"] = True
    dev_index = torch.cuda.current_device() if device is None else int(device)
    env = FlexibleGymEnv(rsc, yaml.safe_dump(cfg, default_flow_style=False, width=float("inf")), device=dev_index)
    env.init()
    policy = load_policy(model_or_policy, torch.device("cuda", dev_index))
    mu_rows = np.repeat([c[0] for c in conditions], E)
    coeff = contact_material(mu_rows if mu_warm is None else np.full(n, mu_warm))
    env.SetContactCoefficient(coeff)
    ev = PolicyEvaluator(env, policy, np.repeat([c[1] for c in conditions], E), np.full(n, float(cmd)), cmd_hz=cmd_hz, vel_hz=vel_hz, act_hz=act_hz, clip=clip)
    post = -(-frames // bucket_steps)
    # the origin one bucket in front of the kick: bucket 0 = steps warm_steps - bucket_steps .. warm_steps - 1, the kick fires at tau = bucket_steps
    ev.set_scenario(stat_buckets=1 + post, stat_every=bucket_steps, t0=warm_steps - bucket_steps, kicks=kicks, kick_first=bucket_steps, gait=gait)
    if warm_steps > bucket_steps:
        ev.run(warm_steps - bucket_steps, accumulate=False, persistent=persistent)
    ev.run(bucket_steps, persistent=persistent)
    if mu_warm is not None:                                    # (the setter's copy is ordered on the pool's stream, behind the warm-up)
        env.SetContactCoefficient(contact_material(mu_rows))
    want_body = record_body or ensemble is not None or recurrence is not None
    chunk = frames if frame_chunk is None else min(frame_chunk, frames)
    body_parts, ens_parts, rec = [], [], None
    for first in range(0, frames, chunk):
        rec = None                                             # the previous call's recorder goes back to the allocator before this call's is taken
        rec = ev.run(min(chunk, frames - first), record=("body",) if want_body else (), persistent=persistent)
        if ensemble is not None and not ensemble_survivors:
            ens_parts.append(ensemble_to_numpy(ensemble_device(rec["body"], len(conditions), ensemble)))
        if record_body:
            body_parts.append(rec["body"].cpu().numpy())
    st = ev.bucket_statistics()
    gt = ev.bucket_gait_statistics(mass, g) if gait else None
    body = (body_parts[0] if len(body_parts) == 1 else np.concatenate(body_parts, 0)) if record_body else None
    ens = None
    if ensemble is not None:
        if ensemble_survivors:                                 # (one chunk: rec is the whole run's recorder)
            up = torch.from_numpy((st["falls"][1:].sum(0) == 0).astype(np.uint8)).to(ev.dev)
            ens_parts.append(ensemble_to_numpy(ensemble_device(rec["body"], len(conditions), ensemble, mask=up)))
        ens = {k: (None if ens_parts[0][k] is None else np.concatenate([p[k] for p in ens_parts], 1)) for k in ens_parts[0]}
    rqa = None
    if recurrence is not None:                                 # (one chunk: rec is the whole run's recorder)
        res = recurrence_to_numpy(recurrence_device(rec["body"], recurrence, frame_first=frames - T_rec, frames=T_rec, lags=T_rec // 2 + 1))
        rqa = recurrence_measures(res["counts"], T_rec, recurrence)
        per = recurrence_period(res["lag"], T_rec, max(recurrence["theiler"], 1), ev._dt)
        rqa.update(period_s=per["period_s"], period_fraction=per["period_fraction"], kept=res["counts"][:, 0].astype(np.int64))
    rec = None
    out = []
    for i, (m, d) in enumerate(conditions):
        sl = slice(i * E, (i + 1) * E)
        falls = st["falls"][1:, sl].sum(0)
        row = dict(mu=m, delay=d, cmd=float(cmd), explorations=E, surviving=float(np.mean(falls == 0)), falls=falls, stats={k: v[:, sl] for k, v in st.items()},
                   kicks=kicks[sl])
        if record_body:
            row["body"] = body[:, sl]
        if gait:
            row["gait"] = {k: v[:, sl] for k, v in gt.items()}
        if ens is not None:
            row["ensemble"] = ensemble_row(ens, i, ev._dt)
        if rqa is not None:
            row["recurrence"] = {k: v[sl] for k, v in rqa.items()}
        out.append(row)
    return out


def perturbation_table(rows, gait=False, ensemble=False, recurrence=False):
    """one line per (mu, delay) of a perturbation_study: the surviving fraction, and the ensemble mean of v_x / z / pitch of the survivors in the
    bucket in front of the kick and in the last one; gait (rows of a study with gait=True): the cost of transport and the mean duty factor too;
    ensemble (rows of a study with an ensemble spec): the entropy of the first and of the last frame, its decay rate kappa (nats/s) and the
    time at which it reaches its floor (entropy_rate; NaN for fewer than 3 frames); recurrence (rows of a study with a recurrence spec): the
    medians over the survivors of RR, DET, LMAX and period_s"""
    out = ["%-6s %-5s %-5s %-5s %-9s " % ("mu", "delay", "cmd", "E", "surviving") + " ".join("%-12s" % k for k in ("vx_before", "vx_last", "z_before", "z_last",
                                                                                                              "pitch_before", "pitch_last"))]
    if gait:
        out[0] += " " + " ".join("%-12s" % k for k in ("cot_before", "cot_last", "duty_before", "duty_last"))
    if ensemble:
        out[0] += " " + " ".join("%-12s" % k for k in ("H0", "H_last", "kappa", "t_floor"))
    if recurrence:
        out[0] += " " + " ".join("%-12s" % k for k in RECURRENCE_TABLE_KEYS)
    for r in rows:
        up = r["falls"] == 0
        m = lambda k, b: float(r["stats"][k][b, up].mean()) if up.any() else float("nan")
        out.append("%-6g %-5d %-5g %-5d %-9.4f " % (r["mu"], r["delay"], r["cmd"], r["explorations"], r["surviving"])
                   + " ".join("%+12.4f" % m(k, b) for k in ("vx_body_mean", "z_mean", "pitch_mean") for b in (0, -1)))
        if gait:
            gm = lambda keys, b: float(np.nanmean(np.stack([r["gait"][k][b, up] for k in keys]))) if up.any() else float("nan")
            out[-1] += " " + " ".join("%+12.4f" % gm(keys, b) for keys in (("cot",), ("duty0", "duty1", "duty2", "duty3")) for b in (0, -1))
        if ensemble:
            e = r["ensemble"]
            fit = entropy_rate(e["t"], e["entropy"], stride=max(1, len(e["t"]) // 500)) if len(e["t"]) >= 3 else dict(kappa=float("nan"), t_floor=float("nan"))
            out[-1] += " " + " ".join("%+12.4f" % v for v in (e["entropy"][0], e["entropy"][-1], fit["kappa"], fit["t_floor"]))
        if recurrence:
            med = lambda v: float(np.nanmedian(v[up])) if up.any() and np.any(np.isfinite(v[up])) else float("nan")
            out[-1] += " " + " ".join("%+12.4f" % med(r["recurrence"][k]) for k in RECURRENCE_TABLE_KEYS)
    return "\n".join(out)


RECURRENCE_TABLE_KEYS = ("RR", "DET", "LMAX", "period_s")


FOOTFALL_TABLE_KEYS = ("stride_hz_db", "duty_db", "gait", "sat_max")


CORRELATION_TABLE_KEYS = ("corr_max", "corr_leg", "corr_unit")


def spectrum_table_keys(sources=None):
    """the columns sweep_table(spectrum=...) adds: vib_peak_hz_<source>, vib_frac_<source> per source (None: all of SPECTRUM_SOURCES)"""
    return tuple(k + name for name in (tuple(SPECTRUM_SOURCES) if sources is None else sources) for k in ("vib_peak_hz_", "vib_frac_"))


def sweep_table(rows, gait=False, recurrence=False, footfall=False, correlation=False, spectrum=False):
    """one line per row of a robustness_sweep; gait (rows of a sweep with gait=True): the cost of transport, the mean mechanical power, the four
    duty factors, `stride_hz` (mean over the legs of gait_from_sums' stride_hz<l>: the RAW contact flags' touchdown rate, several times the
    stride frequency because the flag chatters while a foot is down -- the debounced one is stride_hz_db) and the flight fraction too; footfall
    (rows of a sweep with a footfall spec): stride_hz_db and duty_db, the debounced stride frequency and duty factor (footfall_row, mean over
    the legs), the gait's name and, with a motor spec too, sat_max, the largest saturated fraction of a joint; recurrence (rows of a sweep with a recurrence spec): the
    recurrence rate, the determinism, the longest diagonal line and the stride period too; correlation (rows of a sweep with correlation=...):
    corr_max, the largest |r| of a pair, with corr_leg and corr_unit, the x and the y column it belongs to; spectrum (True, or the tuple of
    sources; rows of a sweep with spectrum=...): per source vib_peak_hz_<source>, the frequency of the Welch spectrum's largest bin without
    bin 0, and vib_frac_<source>, the fraction of its power above the band (spectrum_row)"""
    keys = ("vx_body_mean", "vx_body_std", "z_mean", "z_std", "roll_std", "pitch_mean", "pitch_std", "yaw_rate_mean")
    staircase = bool(rows) and "level" in rows[0]              # one row per (condition, level): the level and its commanded v_x as well
    lead = ("mu", "delay", "cmd") + (("level", "cmd_level") if staircase else ()) + ("falls",)
    out = [" ".join("%-*s" % (9 if k == "cmd_level" else 6 if k == "mu" else 5, k) for k in lead) + " " + " ".join("%-12s" % k for k in keys)]
    gkeys = ("cot", "power_mean", "duty0", "duty1", "duty2", "duty3", "stride_hz", "flight")
    if gait:
        out[0] += " " + " ".join("%-12s" % k for k in gkeys)
    if recurrence:
        out[0] += " " + " ".join("%-12s" % k for k in RECURRENCE_TABLE_KEYS)
    if footfall:
        out[0] += " " + " ".join("%-12s" % k for k in FOOTFALL_TABLE_KEYS)
    if correlation:
        out[0] += " " + " ".join("%-12s" % k for k in CORRELATION_TABLE_KEYS)
    vkeys = spectrum_table_keys(None if spectrum is True else spectrum) if spectrum else ()
    if spectrum:
        out[0] += " " + " ".join("%-12s" % k for k in vkeys)
    for r in rows:
        lvl = "%-5d %-9g " % (r["level"], r["cmd_level"]) if staircase else ""
        out.append("%-6g %-5d %-5g %s%-5d " % (r["mu"], r["delay"], r["cmd"], lvl, r["falls"]) + " ".join("%+12.4f" % r[k] for k in keys))
        if gait:
            g = dict(r, stride_hz=float(np.mean([r["stride_hz%d" % l] for l in range(4)])))
            out[-1] += " " + " ".join("%+12.4f" % g[k] for k in gkeys)
        if recurrence:
            out[-1] += " " + " ".join("%+12.4f" % r["recurrence"][k] for k in RECURRENCE_TABLE_KEYS)
        if footfall:
            sat = float(np.nanmax(r["motor"]["saturated"])) if "motor" in r and not np.all(np.isnan(r["motor"]["saturated"])) else float("nan")
            out[-1] += " %+12.4f %+12.4f %-12s %+12.4f" % (r["footfall"]["stride_hz"], r["footfall"]["duty"], r["footfall"]["gait"], sat)
        if correlation:
            label = lambda v: "-" if v is None else v if isinstance(v, str) else ":".join(str(p) for p in v)
            out[-1] += " %+12.4f %-12s %-12s" % (r["corr_max"], label(r["corr_leg"]), label(r["corr_unit"]))
        if spectrum:
            out[-1] += " " + " ".join("%+*.4f" % (max(12, len(k)), r[k]) for k in vkeys)
    return "\n".join(out)
