"""Entry-wise parity of the rigid-body dynamics: shared by tests/test_dynamics_parity_reference.py (CPU: the f32 build of the oracle
and the host emulation of the kernel source) and tests/test_gpu_dynamics_parity.py (the HIP kernels on an MI355X).

What is compared, always against the f64 build of the oracle on ONE identical, f32-rounded state:
  the probe   M^-1 (18 x 18) and the bias b (18) of the current state (GetInverseMassMatrix / GetNonlinear), entry by entry;
  the step    gv_after - gv_before of one env step in free flight: one substep (dt M^-1 (tau - b) itself) or the config's eight.

Metrics (dimensionless, per robot; d_i = M^-1_ii of the f64 oracle):
  minv        |dM^-1_ij| / sqrt(d_i d_j)                -- M^-1 is symmetric positive definite, so |M^-1_ij| <= sqrt(d_i d_j): every entry
                                                           is bounded by 1 in this scaling whatever its units; reported per block
  bias        |db_j| sqrt(d_j) / sqrt(b' M^-1 b)        -- the error seen as the acceleration it causes, relative to the robot's whole
                                                           bias acceleration
  inc1, inc8  sqrt(e' M e) / sqrt(dv' M dv), e = dv_cand - dv_f64, M = inv(M^-1_f64) at the start state; the per-dof terms
              |e_j| / sqrt(d_j) over the same denominator locate a failure

BOUND[family][metric] = 8 x the worst error of the F32 BUILD OF THE ORACLE (OracleVecEnv(cfg, precision="f32")) against the f64 build
on that family's inputs, rounded up to one significant digit (`reference_errors()` re-measures it; test_dynamics_parity_reference.py
holds the table to it).  The reference sets the bound, never the kernels: the kernels are the same f32 arithmetic in another order
(-ffp-contract=on, one-ulp v_rcp / v_rsq for divisions, the Schur-complement elimination order, the lane reduction order), and 8 x
leaves room for that while it still refuses a 1e-4 relative error.
The f64 oracle's getters return float32: a floor of half an ulp, ~6e-8 relative per entry, on the reference side of the probe.
It is inside the f32 oracle's measured error (>= 5e-7 in every metric below) and therefore inside every bound.
"""
import functools

import numpy as np

import _np_robot as R
import oracle as O
import parity_lib as PL
from conftest import load_env_cfg

S = O.S
GC, GV = S["GC"], S["GV"]
LIN, ANG, JNT = slice(0, 3), slice(3, 6), slice(6, 18)
BLOCKS = (("lin-lin", LIN, LIN), ("ang-ang", ANG, ANG), ("jnt-jnt", JNT, JNT), ("lin-ang", LIN, ANG), ("lin-jnt", LIN, JNT), ("ang-jnt", ANG, JNT))
DOF = ["vx", "vy", "vz", "wx", "wy", "wz"] + ["%s.%s" % (leg, j) for leg in ("FR", "FL", "HR", "HL") for j in ("abad", "hip", "knee")]


def block_of(i, j):
    kind = lambda k: "lin" if k < 3 else ("ang" if k < 6 else "jnt")
    a, b = sorted((kind(i), kind(j)), key=("lin", "ang", "jnt").index)
    return "%s-%s" % (a, b)


# ---------------------------------------------------------------------------------------------------------------- state families
# A family writes the GC / GV slots of a pool state, robot by robot IN ORDER from its own fixed seed: robot i of a pool of 5 is robot
# i of a pool of 48 (the model parameters of a pool are keyed by the env id in the same way), every leg of a robot has another pose
# (a leg swap shows) and so has every robot of a wave (a robot swap shows).
NOMINAL_JOINTS = np.array([0.0, -0.78, 1.57] * 4)
# The range the task can reach.  Position targets are action + nominal pose with |action| <= 1 (env_step: p = action * 1.0 + nominal,
# abad 0 in every shipped config; the policy's actions are clipped to +-1), so abduction reaches +-1 rad, the hip -1.78 .. 0.22 and
# the knee up to 2.57 (folded).  The knee's lower end is the gait generator's: inverse_kinematics caps the reach at
# l_thigh + l_calf - 1e-4, a nearly straight leg (knee ~0.03 rad); 0 is the limit of that.
JOINT_LO = np.array([-1.0, -1.78, 0.0] * 4)
JOINT_HI = np.array([1.0, 0.22, 2.57] * 4)
MAX_JOINT_RATE, MAX_BASE_RATE, MAX_BASE_SPEED = 40.0, 10.0, 3.0          # the motor's no-load speed (MotorMaxSpeed of the evaluation config); rad/s; m/s


def _quat(axis, deg):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    half = 0.5 * np.radians(deg)
    return np.concatenate([[np.cos(half)], np.sin(half) * axis])


# members 5 and 6 are ONE rotation (120 degrees about (1, 1, 1)) as -q and +q: w = -0.5 and +0.5
ATTITUDES = [_quat([0, 0, 1], 0.0), _quat([1, 0, 0], 90.0), _quat([0, 1, 0], 90.0), _quat([0, 0, 1], 90.0), _quat([1, 2, -2], 179.0),
             -_quat([1, 1, 1], 120.0), _quat([1, 1, 1], 120.0)]


def attitude_twins(n):
    """-> [(i, i + 1)]: robots of the `attitude` family that differ in the sign of the quaternion alone"""
    return [(i, i + 1) for i in range(n - 1) if i % len(ATTITUDES) == 5]


def _velocity(rng, scale):
    return scale * np.concatenate([rng.uniform(-MAX_BASE_SPEED, MAX_BASE_SPEED, 3), rng.uniform(-MAX_BASE_RATE, MAX_BASE_RATE, 3),
                                   rng.uniform(-MAX_JOINT_RATE, MAX_JOINT_RATE, 12)])


def nominal(st, rng):
    """random poses about the nominal stance (joints +-0.4 rad, each on its own), base tilted at random, at rest"""
    st = st.copy()
    for i in range(st.shape[0]):
        st[i, GC:GC + 19] = R.random_config(rng)
        st[i, GV:GV + 18] = 0.0
    return PL.f32_round_state(st)


def joint_range(st, rng):
    """every joint within 0.02 rad of one END of JOINT_LO .. JOINT_HI, the four legs of a robot at four different ones of the eight corners
    (so abduction of both signs within a robot); every fourth robot has all four knees nearly straight (0 .. 0.05 rad, each another
    value), the one behind it all four folded (2.57 - U(0, 0.05)); at rest"""
    st = st.copy()
    for i in range(st.shape[0]):
        gc = R.random_config(rng)
        corner = rng.permutation(8)[:4]
        high = np.array([[(c >> k) & 1 for k in range(3)] for c in corner]).reshape(12) == 1
        inward = rng.uniform(0.0, 0.02, 12)
        q = np.where(high, JOINT_HI - inward, JOINT_LO + inward)
        straight, folded = rng.uniform(0.0, 0.05, 4), JOINT_HI[2] - rng.uniform(0.0, 0.05, 4)
        if i % 4 == 0:
            q[2::3] = straight
        elif i % 4 == 1:
            q[2::3] = folded
        gc[7:19] = q
        st[i, GC:GC + 19] = gc
        st[i, GV:GV + 18] = 0.0
    return PL.f32_round_state(st)


def attitude(st, rng):
    """base attitudes ATTITUDES[i % 7]: identity, 90 degrees about x, y and z, 179 degrees about (1, 2, -2), and one rotation as -q and
    as +q -- that pair (attitude_twins) shares everything else, the model parameters too, and must give the same result to rounding; half-range velocities"""
    st = st.copy()
    for i in range(st.shape[0]):
        m = i % len(ATTITUDES)
        gc, gv = R.random_config(rng), _velocity(rng, 0.5)
        if m == 6 and i > 0:
            st[i] = st[i - 1]                   # the whole row: a pool with a randomised model keeps the inertias in its state
            gc, gv = st[i - 1, GC:GC + 19].copy(), st[i - 1, GV:GV + 18].copy()
        gc[3:7] = ATTITUDES[m]
        st[i, GC:GC + 19] = gc
        st[i, GV:GV + 18] = gv
    return PL.f32_round_state(st)


def moving(st, rng):
    """random poses with joint rates up to +-40 rad/s, base angular rate up to +-10 rad/s, base velocity up to +-3 m/s, scaled by
    0, 1/2 and 1 by robot"""
    st = st.copy()
    for i in range(st.shape[0]):
        st[i, GC:GC + 19] = R.random_config(rng)
        st[i, GV:GV + 18] = _velocity(rng, (0.0, 0.5, 1.0)[i % 3])
    return PL.f32_round_state(st)


def one_hot_rate(st, rng):
    """random poses; robot i has ONE nonzero velocity: joint i % 15 at +-30 rad/s, or (i % 15 = 12, 13, 14) one base angular-rate
    component at +-10 rad/s"""
    st = st.copy()
    for i in range(st.shape[0]):
        st[i, GC:GC + 19] = R.random_config(rng)
        gv = np.zeros(18)
        k, sign = i % 15, (1.0 if (i // 15) % 2 == 0 else -1.0)
        if k < 12:
            gv[6 + k] = 30.0 * sign
        else:
            gv[3 + k - 12] = MAX_BASE_RATE * sign
        st[i, GV:GV + 18] = gv
    return PL.f32_round_state(st)


def far_away(st, rng):
    """random poses and half-range velocities with the base at x, y = +-250 m (the four sign pairs by robot): M^-1 and b must be those
    of the same pose at the origin"""
    st = st.copy()
    for i in range(st.shape[0]):
        gc = R.random_config(rng)
        gc[0:2] += [250.0 * (1 if i % 2 == 0 else -1), 250.0 * (1 if (i // 2) % 2 == 0 else -1)]
        st[i, GC:GC + 19] = gc
        st[i, GV:GV + 18] = _velocity(rng, 0.5)
    return PL.f32_round_state(st)


FAMILIES = dict(nominal=nominal, joint_range=joint_range, attitude=attitude, moving=moving, one_hot_rate=one_hot_rate, far_away=far_away)
SEED = dict(nominal=101, joint_range=102, attitude=103, moving=104, one_hot_rate=105, far_away=106)


def family_state(template, family):
    """the family's pool state on top of `template` (a pool's own get_state(): model parameters, task state)"""
    return FAMILIES[family](np.array(template, np.float64), np.random.RandomState(SEED[family]))


# ------------------------------------------------------------------------------------------------------------------------ bounds
# 8 x the f32 oracle's worst error (the number in the comment: measured by reference_errors(), probe on PROBE_CFG at N_REF robots,
# increments at N_INC robots over the POOLS of the family), rounded up to one significant digit.
BOUND = {
    #                     scaled M^-1          bias                 one substep          eight substeps          <- 8 x the measured value behind it
    "nominal":      dict(minv=9e-6,  # 1.06e-6
                         bias=3e-6,  # 2.62e-7
                         inc1=5e-6,  # 5.86e-7
                         inc8=5e-6),  # 6.08e-7
    "joint_range":  dict(minv=2e-5,  # 1.53e-6
                         bias=2e-6,  # 1.88e-7
                         inc1=4e-6,  # 4.75e-7
                         inc8=3e-6),  # 2.57e-7
    "attitude":     dict(minv=9e-6,  # 1.03e-6
                         bias=2e-6),  # 1.81e-7
    # with rates of up to 40 rad/s the increment's error is the rounding of gv itself: half an ulp of 40 rad/s is 1.9e-6 rad/s, on an
    # increment of (without torque) a few 1e-2 rad/s -- the f32 oracle's error relative to the increment is 10-100 x that of a robot at rest
    "moving":       dict(minv=1e-5,  # 1.16e-6
                         bias=2e-6,  # 1.88e-7
                         inc1=4e-4,  # 4.34e-5
                         inc8=2e-4),  # 1.45e-5
    "one_hot_rate": dict(minv=9e-6,  # 1.07e-6
                         bias=2e-6,  # 2.10e-7
                         inc1=5e-4,  # 5.57e-5
                         inc8=2e-4),  # 2.40e-5
    "far_away":     dict(minv=2e-5,  # 1.45e-6
                         bias=2e-6,  # 2.14e-7
                         inc1=6e-5,  # 6.45e-6
                         inc8=3e-5),  # 2.69e-6
}
PROBE_CFG = "default_cfg.yaml"           # per-robot randomised model: every robot of the pool has other inertias
N_REF, N_INC = 48, 24


def round_up_1(x):
    e = int(np.floor(np.log10(x)))
    return float("%de%d" % (int(np.ceil(x / 10.0 ** e * (1 - 1e-12))), e))


# ----------------------------------------------------------------------------------------------------------------------- metrics
def unflatten(minv):
    """[N, 324] column-major (the getters' layout) -> [N, 18, 18] in float64"""
    return np.asarray(minv, np.float64).reshape(-1, 18, 18).transpose(0, 2, 1)


def minv_scaled_error(minv_ref, minv_c, scale=None):
    """-> [N, 18, 18]: |dM^-1_ij| / sqrt(d_i d_j), d from the reference (or from `scale`, an f64 M^-1)"""
    d = np.sqrt(np.einsum("nii->ni", minv_ref if scale is None else scale))
    return np.abs(minv_c - minv_ref) / (d[:, :, None] * d[:, None, :])


def bias_scaled_error(minv_ref, b_ref, b_c, scale=None):
    """-> [N, 18]; `scale`: (M^-1, b) of the f64 oracle where the reference side is not the f64 oracle itself"""
    minv_s, b_s = (minv_ref, b_ref) if scale is None else scale
    d = np.sqrt(np.einsum("nii->ni", minv_s))
    den = np.sqrt(np.einsum("ni,nij,nj->n", b_s, minv_s, b_s))
    return np.abs(np.asarray(b_c, np.float64) - b_ref) * d / den[:, None]


def increment_errors(minv_ref, dv_ref, dv_c):
    """-> (energy-norm error [N], per-dof terms [N, 18]), both over sqrt(dv' M dv) of the reference"""
    M = np.linalg.inv(minv_ref)
    e = dv_c - dv_ref
    den = np.sqrt(np.einsum("ni,nij,nj->n", dv_ref, M, dv_ref))
    d = np.sqrt(np.einsum("nii->ni", minv_ref))
    return np.sqrt(np.einsum("ni,nij,nj->n", e, M, e)) / den, np.abs(e) / d / den[:, None]


def _block_max(E):
    """[N, 18, 18] -> {block: (value, robot, i, j)}, both triangles of the coupling blocks"""
    out = {}
    for name, a, b in BLOCKS:
        best = (-1.0, 0, 0, 0)
        for ra, rb in ((a, b), (b, a)):
            sub = E[:, ra, rb]
            n, i, j = np.unravel_index(np.argmax(sub), sub.shape)
            if sub[n, i, j] > best[0]:
                best = (float(sub[n, i, j]), int(n), int(i + ra.start), int(j + rb.start))
        out[name] = best
    return out


def assert_probe_entrywise(minv_ref, b_ref, minv_c, b_c, family, label="probe", symmetry=True, scale=None):
    """arrays: [N, 18, 18] f64 reference M^-1, [N, 18] reference bias, the candidate's.  -> {block or "bias" or "symmetry": error / BOUND}"""
    bound = BOUND[family]
    ratios, fails = {}, []
    for name, (val, n, i, j) in _block_max(minv_scaled_error(minv_ref, minv_c, None if scale is None else scale[0])).items():
        ratios[name] = val / bound["minv"]
        if not val <= bound["minv"]:
            fails.append("M^-1 block %s: robot %d entry (%d %s, %d %s) scaled error %.3g > %.1g (candidate %.9g, f64 %.9g)"
                         % (name, n, i, DOF[i], j, DOF[j], val, bound["minv"], minv_c[n, i, j], minv_ref[n, i, j]))
    if symmetry:
        d = np.sqrt(np.einsum("nii->ni", minv_ref))
        A = np.abs(minv_c - minv_c.transpose(0, 2, 1)) / (d[:, :, None] * d[:, None, :])
        n, i, j = np.unravel_index(np.argmax(A), A.shape)
        ratios["symmetry"] = float(A[n, i, j]) / bound["minv"]
        if not A[n, i, j] <= bound["minv"]:
            fails.append("M^-1 symmetry, block %s: robot %d entries (%d %s, %d %s) differ by %.3g (scaled) > %.1g"
                         % (block_of(i, j), n, i, DOF[i], j, DOF[j], A[n, i, j], bound["minv"]))
    B = bias_scaled_error(minv_ref, b_ref, b_c, scale)
    n, j = np.unravel_index(np.argmax(B), B.shape)
    ratios["bias"] = float(B[n, j]) / bound["bias"]
    if not B[n, j] <= bound["bias"]:
        fails.append("bias: robot %d dof %d %s scaled error %.3g > %.1g (candidate %.9g, f64 %.9g)"
                     % (n, j, DOF[j], B[n, j], bound["bias"], np.asarray(b_c)[n, j], b_ref[n, j]))
    print("[%s %s] error / BOUND: %s" % (label, family, ", ".join("%s %.3f" % kv for kv in ratios.items())))
    assert not fails, "%s, family %s:\n  " % (label, family) + "\n  ".join(fails)
    return ratios


def assert_increment(minv_ref, dv_ref, dv_c, family, key, label="increment"):
    """-> {"energy": error / BOUND, "lin" / "ang" / "jnt": the per-dof terms / BOUND}"""
    bound = BOUND[family][key]
    en, per = increment_errors(minv_ref, dv_ref, dv_c)
    n = int(np.argmax(en))
    j = int(np.argmax(per[n]))
    ratios = {"energy": float(en[n]) / bound}
    for name, sl in (("lin", LIN), ("ang", ANG), ("jnt", JNT)):
        ratios[name] = float(per[:, sl].max()) / bound
    print("[%s %s %s] error / BOUND: %s" % (label, family, key, ", ".join("%s %.3f" % kv for kv in ratios.items())))
    assert en[n] <= bound, ("%s, family %s, %s: robot %d energy-norm error %.3g > %.1g; largest per-dof term %.3g at dof %d %s (block %s): "
                            "increment candidate %.9g, f64 %.9g" % (label, family, key, n, en[n], bound, per[n, j], j, DOF[j], block_of(j, j)[:3],
                                                                    dv_c[n, j], dv_ref[n, j]))
    return ratios


def oracle_probe(orc):
    return unflatten(orc.inverse_mass_matrix()), orc.nonlinear().astype(np.float64)


def candidate_probe(cand):
    """the candidate's (M^-1 [N, 18, 18], b [N, 18]) in float64; an OracleVecEnv (the f32 build) counts as a candidate"""
    if hasattr(cand, "probe"):
        minv, b = cand.probe()
    else:
        minv, b = cand.inverse_mass_matrix(), cand.nonlinear()
    return unflatten(minv), np.asarray(b, np.float64)


def check_probe_entrywise(orc, cand, family, label="probe"):
    """Both pools hold ONE identical state (set_state of the same f32-rounded array).  Every entry of the candidate's M^-1 and bias
    within BOUND[family] of the f64 oracle's, M^-1 symmetric within the same bound; for `far_away` also against the f64 oracle with
    the base moved to x = y = 0; for `attitude` the -q / +q twins against each other.  -> the ratios error / BOUND."""
    st = orc.get_state()
    assert np.array_equal(st[:, 0:37], cand.get_state()[:, 0:37]), "check_probe_entrywise needs both pools in one identical state"
    minv_ref, b_ref = oracle_probe(orc)
    minv_c, b_c = candidate_probe(cand)
    ratios = assert_probe_entrywise(minv_ref, b_ref, minv_c, b_c, family, label)
    if family == "far_away":
        home = st.copy()
        home[:, GC:GC + 2] = 0.0
        orc.set_state(home)
        minv_0, b_0 = oracle_probe(orc)
        orc.set_state(st)
        ratios["at_origin"] = max(assert_probe_entrywise(minv_0, b_0, minv_c, b_c, family, label + " vs the pose at the origin").values())
    if family == "attitude":
        a, b = [np.array(x) for x in zip(*attitude_twins(orc.n))] if attitude_twins(orc.n) else (np.zeros(0, int), np.zeros(0, int))
        if len(a):
            assert np.array_equal(st[a, GC + 3:GC + 7], -st[b, GC + 3:GC + 7]) and np.array_equal(st[a, GC + 7:GC + 37], st[b, GC + 7:GC + 37])
            assert np.array_equal(st[a, S["MATERIAL"]:S["OB"]], st[b, S["MATERIAL"]:S["OB"]])
            # the candidate's -q robot against its own +q robot, scaled by the f64 oracle's values
            ratios["twins"] = max(assert_probe_entrywise(minv_c[a], b_c[a], minv_c[b], b_c[b], family, label + " -q against +q", symmetry=False,
                                                         scale=(minv_ref[a], b_ref[a])).values())
    return ratios


# ------------------------------------------------------------------------------------------------------ pools of the increment check
# All in free flight: base at 0.55 m, tilt (rotation vector) at most 0.5 rad -- inside the termination cone (cos > 0.5) --, no toe
# within reach of the ground, INCONTACT and the stored impulses cleared.  Torque patterns: "zero" (Stiffness = Damping = 0: tau = 0,
# the increment is the bias acceleration alone), "random" (the config's gains, actions N(0, 0.5) clipped to +-1), "one_joint" (one
# joint's target at +-1, the others at their current angle: tau is one-hot up to the damping of a moving joint, the increment a
# column of M^-1).  substeps 1: control_dt = simulation_dt (run-time-setting kernels on the device), 8: the config's own control_dt.
# (config, torque pattern, substeps, family); `attitude` is left out: its members lie outside the termination cone.
POOLS = [
    ("bp5_imitation.yaml", "zero", 1, "moving"), ("bp5_imitation.yaml", "zero", 8, "moving"),
    ("bp5_imitation.yaml", "random", 1, "moving"), ("bp5_imitation.yaml", "random", 8, "moving"),
    ("bp5_imitation.yaml", "one_joint", 1, "nominal"), ("bp5_imitation.yaml", "one_joint", 8, "nominal"),
    ("default_cfg.yaml", "zero", 1, "one_hot_rate"), ("default_cfg.yaml", "zero", 8, "one_hot_rate"),
    ("default_cfg.yaml", "random", 1, "joint_range"), ("default_cfg.yaml", "random", 8, "joint_range"),
    ("default_cfg.yaml", "one_joint", 1, "far_away"), ("default_cfg.yaml", "one_joint", 8, "far_away"),
    ("bp5_terrain.yaml", "zero", 1, "nominal"), ("bp5_terrain.yaml", "zero", 8, "one_hot_rate"),
    ("bp5_terrain.yaml", "random", 1, "moving"), ("bp5_terrain.yaml", "random", 8, "moving"),
    ("bp5_terrain.yaml", "one_joint", 1, "one_hot_rate"), ("bp5_terrain.yaml", "one_joint", 8, "nominal"),
]


def pool_id(pool):
    return "%s-%s-%dsub-%s" % (pool[0].split(".")[0], pool[1], pool[2], pool[3])


def pool_cfg(pool, n):
    name, torque, substeps, _ = pool
    cfg = load_env_cfg(name, num_envs=n)
    if torque == "zero":
        cfg.update(Stiffness=0.0, Damping=0.0)
    if substeps == 1:
        cfg.update(control_dt=cfg["simulation_dt"])
    assert int(round(cfg["control_dt"] / cfg["simulation_dt"])) == substeps
    return cfg


def flight_state(template, family):
    """the family's state put into free flight (see POOLS)"""
    st = family_state(template, family)
    rng = np.random.RandomState(SEED[family] + 1000)
    for i in range(st.shape[0]):
        rv = rng.normal(size=3)
        rv *= rng.uniform(0.0, 0.5) / np.linalg.norm(rv)
        ang = np.linalg.norm(rv)
        st[i, GC + 2] = 0.55
        st[i, GC + 3:GC + 7] = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * rv / ang])
        st[i, S["PTL"]:S["PTL"] + 12] = st[i, GC + 7:GC + 19]
    for key, width in (("TQL", 12), ("TQ", 12), ("LAMW", 12), ("INCONTACT", 4)):
        st[:, S[key]:S[key] + width] = 0.0
    return PL.f32_round_state(st)


def pool_actions(torque, st):
    n = st.shape[0]
    rng = np.random.RandomState(7)
    if torque == "one_joint":
        a = st[:, GC + 7:GC + 19] - NOMINAL_JOINTS
        for i in range(n):
            a[i, i % 12] = 1.0 if (i // 12) % 2 == 0 else -1.0
        return a.astype(np.float32)
    return PL.random_actions(rng, n, 0.5)


def step_increment(env, st, actions):
    """set_state, one step, get_state -> gv_after - gv_before; no robot may end its episode or touch the ground"""
    env.set_state(st)
    _, _, done, _ = env.step(actions)
    after = env.get_state()
    assert not np.asarray(done).any(), "an episode ended: robots %s" % np.nonzero(done)[0]
    assert not after[:, S["INCONTACT"]:S["INCONTACT"] + 4].any(), "a toe touched the ground"
    return after[:, GV:GV + 18] - st[:, GV:GV + 18], after


def check_substep_increment(make_orc, make_cand, cfg, family, actions, label="increment"):
    """`cfg`: a pool_cfg; `actions`: a torque pattern of pool_actions or an [N, 12] array.  -> (ratios, the candidate's state behind the step)"""
    orc, cand = make_orc(cfg), make_cand(cfg)
    st = flight_state(orc.get_state(), family)
    if isinstance(actions, str):
        actions = pool_actions(actions, st)
    orc.set_state(st)
    minv_ref, _ = oracle_probe(orc)
    dv_ref, _ = step_increment(orc, st, actions)
    dv_c, after = step_increment(cand, st, actions)
    key = "inc%d" % int(round(cfg["control_dt"] / cfg["simulation_dt"]))
    return assert_increment(minv_ref, dv_ref, dv_c, family, key, label), (cand, st, actions, after)


# --------------------------------------------------------------------------------------------------------- the reference's own error
def _f32(cfg):
    return O.OracleVecEnv(cfg, precision="f32")


@functools.lru_cache(maxsize=None)
def reference_errors():
    """-> {family: {metric: worst error of the f32 build of the oracle against the f64 build}}: what BOUND is 8 x of"""
    out = {f: {} for f in FAMILIES}
    cfg = load_env_cfg(PROBE_CFG, num_envs=N_REF)
    o64, o32 = O.OracleVecEnv(cfg), _f32(cfg)
    for fam in FAMILIES:
        st = family_state(o64.get_state(), fam)
        o64.set_state(st)
        o32.set_state(st)
        (minv_ref, b_ref), (minv_c, b_c) = oracle_probe(o64), candidate_probe(o32)
        out[fam]["minv"] = float(minv_scaled_error(minv_ref, minv_c).max())
        out[fam]["bias"] = float(bias_scaled_error(minv_ref, b_ref, b_c).max())
    for pool in POOLS:
        cfg = pool_cfg(pool, N_INC)
        o64, o32 = O.OracleVecEnv(cfg), _f32(cfg)
        st = flight_state(o64.get_state(), pool[3])
        a = pool_actions(pool[1], st)
        o64.set_state(st)
        minv_ref, _ = oracle_probe(o64)
        dv_ref, dv_c = step_increment(o64, st, a)[0], step_increment(o32, st, a)[0]
        key = "inc%d" % pool[2]
        out[pool[3]][key] = max(out[pool[3]].get(key, 0.0), float(increment_errors(minv_ref, dv_ref, dv_c)[0].max()))
    return out


if __name__ == "__main__":
    for fam, row in reference_errors().items():
        print("%-13s %s" % (fam, "  ".join("%s %.3g -> %.0e" % (k, v, round_up_1(8 * v)) for k, v in row.items())))
