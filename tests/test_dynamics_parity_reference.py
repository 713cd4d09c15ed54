"""CPU side of the entry-wise dynamics parity (dynamics_parity_lib.py): the bound table is tied to the f32 build of the oracle, the
checks are shown to fail on a 1e-4 relative error that the old max-norm check accepts, the f64 oracle is held to first principles on
the new state families, and the host emulation of the kernel source -- 4-lane, and the 16-lane substep with its own algebra -- passes
every probe family and every increment pool."""
import numpy as np
import pytest

import oracle as O
import _np_robot as R
import parity_lib as PL
import dynamics_parity_lib as DL
from conftest import load_env_cfg
from host_emulation import emu as E

EMUS = [E.EmuVecEnv, E.EmuVecEnv16]


def test_every_bound_is_eight_times_the_f32_oracles_own_error():
    ref = DL.reference_errors()
    assert set(ref) == set(DL.BOUND) == set(DL.FAMILIES)
    for fam, row in ref.items():
        assert set(row) == set(DL.BOUND[fam]), fam
        for metric, err in row.items():
            bound = DL.BOUND[fam][metric]
            print("%-13s %-5s f32 oracle %.3g  bound %.0e  ratio %.3f" % (fam, metric, err, bound, err / bound))
            assert bound / 16 <= err <= bound / 4, (fam, metric, err, bound)
            assert bound == DL.round_up_1(bound)                    # one significant digit
    assert {p[3] for p in DL.POOLS} == {f for f in DL.FAMILIES if "inc1" in DL.BOUND[f]}
    assert {(p[0], p[1], p[2]) for p in DL.POOLS} == {(c, t, s) for c in ("bp5_imitation.yaml", "default_cfg.yaml", "bp5_terrain.yaml")
                                                       for t in ("zero", "random", "one_joint") for s in (1, 8)}


def test_the_families_reach_what_they_claim():
    st0 = O.OracleVecEnv(load_env_cfg(DL.PROBE_CFG, num_envs=DL.N_REF)).get_state()
    small = O.OracleVecEnv(load_env_cfg(DL.PROBE_CFG, num_envs=5)).get_state()
    for fam in DL.FAMILIES:
        st = DL.family_state(st0, fam)
        assert np.array_equal(DL.family_state(small, fam), st[:5]), fam             # a smaller pool is a prefix (model parameters too)
        q = st[:, 7:19].reshape(-1, 4, 3)
        legs = q[:, :, None, :] - q[:, None, :, :]
        assert np.all(np.abs(legs).max(-1)[:, ~np.eye(4, dtype=bool)] > 1e-3), fam    # every leg of a robot in another pose
        twins = {j for _, j in DL.attitude_twins(len(st))} if fam == "attitude" else set()
        rows = [i for i in range(len(st)) if i not in twins]
        assert len(np.unique(np.round(st[rows, 7:19], 6), axis=0)) == len(rows), fam  # every robot in another pose
    jr = DL.family_state(st0, "joint_range")[:, 7:19]
    assert ((jr[:, 0::3] > 0.97).any(1) & (jr[:, 0::3] < -0.97).any(1)).sum() >= 40                 # abduction of both signs
    assert ((jr[:, 2::3] >= 0) & (jr[:, 2::3] <= 0.05)).sum() >= 16 and (jr[:, 2::3] > 2.5).sum() >= 16
    at = DL.family_state(st0, "attitude")
    a, b = DL.attitude_twins(len(at))[0]
    assert at[a, 3] < 0 and np.array_equal(at[a, 3:7], -at[b, 3:7]) and np.array_equal(at[a, 7:37], at[b, 7:37])
    assert abs(2 * np.degrees(np.arccos(at[4, 3])) - 179.0) < 1e-3
    mv = DL.family_state(st0, "moving")
    assert not mv[0::3, 19:37].any() and np.abs(mv[:, 25:37]).max() > 38.0 and np.abs(mv[:, 22:25]).max() > 9.0 and np.abs(mv[:, 19:22]).max() > 2.7
    oh = DL.family_state(st0, "one_hot_rate")[:, 19:37]
    assert ((oh != 0).sum(1) == 1).all() and set(np.nonzero(oh)[1]) == set(range(3, 18))
    assert (np.abs(DL.family_state(st0, "far_away")[:, 0:2]) > 249.0).all()


class _Arrays(object):
    """the probe interface of check_probe_max_norm over plain arrays"""

    def __init__(self, minv, b):
        self.minv, self.b = minv, b

    def inverse_mass_matrix(self):
        return self.minv

    def nonlinear(self):
        return self.b

    def probe(self):
        return self.minv, self.b


def test_a_planted_1e_4_relative_error_is_refused_and_the_old_check_accepts_it():
    fam = "nominal"
    cfg = load_env_cfg(DL.PROBE_CFG, num_envs=DL.N_REF)
    o64, o32 = O.OracleVecEnv(cfg), O.OracleVecEnv(cfg, precision="f32")
    st = DL.family_state(o64.get_state(), fam)
    o64.set_state(st); o32.set_state(st)
    flat64, b64 = o64.inverse_mass_matrix(), o64.nonlinear()
    flat32, b32 = o32.inverse_mass_matrix(), o32.nonlinear()
    minv_ref, b_ref = DL.oracle_probe(o64)
    DL.assert_probe_entrywise(minv_ref, b_ref, DL.unflatten(flat32), b32.astype(np.float64), fam)         # clean: passes
    PL.check_probe_max_norm(_Arrays(flat64, b64), _Arrays(flat32, b32))
    # one entry per block: the pool's largest of the block in the scaled sense (a 1e-4 relative error there is 1e-4 x its scaled size:
    # the couplings of the base's linear and angular rows are only 0.15 of sqrt(d_i d_j) at most) among those under 0.18 x max |M^-1|
    # (a joint's diagonal, ~110) -- 1e-4 of an entry beyond 0.2 x the maximum is what the max-norm does see
    d = np.sqrt(np.einsum("nii->ni", minv_ref))
    scaled = np.abs(minv_ref) / (d[:, :, None] * d[:, None, :])
    scaled[np.abs(minv_ref) > 0.18 * np.abs(minv_ref).max()] = 0.0
    for name, ra, rb in DL.BLOCKS:
        sub = scaled[:, ra, rb]
        robot, i, j = np.unravel_index(np.argmax(sub), sub.shape)
        i, j = i + ra.start, j + rb.start
        assert 1e-4 * scaled[robot, i, j] > 1.5 * DL.BOUND[fam]["minv"], (name, scaled[robot, i, j])
        bad = flat32.copy().reshape(-1, 18, 18)
        bad[robot, j, i] *= 1.0 + 1e-4                                # column-major: [col, row]
        bad[robot, i, j] = bad[robot, j, i]                           # keep it symmetric: the block check must catch it, not the symmetry check
        bad = bad.reshape(-1, 324)
        PL.check_probe_max_norm(_Arrays(flat64, b64), _Arrays(bad, b32))         # the gap: the old check accepts it
        with pytest.raises(AssertionError, match=r"M\^-1 block %s: robot %d entry \(%d " % (name, robot, min(i, j))) as exc:
            DL.assert_probe_entrywise(minv_ref, b_ref, DL.unflatten(bad), b32.astype(np.float64), fam)
        assert "symmetry" not in str(exc.value) and str(exc.value).count("M^-1 block") == 1
    # an asymmetric candidate
    robot = 7
    bad = flat32.copy().reshape(-1, 18, 18)
    bad[robot, 8, 7] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match="M\\^-1 symmetry, block jnt-jnt: robot %d" % robot):
        DL.assert_probe_entrywise(minv_ref, b_ref, DL.unflatten(bad.reshape(-1, 324)), b32.astype(np.float64), fam)
    # the bias: the joint that carries the largest share of the bias acceleration
    share = np.abs(b_ref[robot]) * np.sqrt(np.diag(minv_ref[robot]))
    j = 6 + int(np.argmax(share[6:]))
    bad_b = b32.astype(np.float64)
    bad_b[robot, j] *= 1.0 + 1e-4
    assert share[j] / np.sqrt(b_ref[robot] @ minv_ref[robot] @ b_ref[robot]) > 0.1
    with pytest.raises(AssertionError, match="bias: robot %d dof %d %s" % (robot, j, DL.DOF[j])):
        DL.assert_probe_entrywise(minv_ref, b_ref, DL.unflatten(flat32), bad_b, fam)
    # the increment of one substep under a one-joint torque: the driven joint's own entry
    pool = ("bp5_imitation.yaml", "one_joint", 1, fam)
    cfg = DL.pool_cfg(pool, 12)
    o64, o32 = O.OracleVecEnv(cfg), O.OracleVecEnv(cfg, precision="f32")
    st = DL.flight_state(o64.get_state(), fam)
    a = DL.pool_actions("one_joint", st)
    o64.set_state(st)
    minv_ref, _ = DL.oracle_probe(o64)
    dv_ref, dv32 = DL.step_increment(o64, st, a)[0], DL.step_increment(o32, st, a)[0]
    DL.assert_increment(minv_ref, dv_ref, dv32, fam, "inc1")
    j = 6 + robot % 12
    bad = dv32.copy()
    bad[robot, j] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match="robot %d energy-norm error .* at dof %d %s " % (robot, j, DL.DOF[j])):
        DL.assert_increment(minv_ref, dv_ref, bad, fam, "inc1")


@pytest.fixture(scope="module")
def f64_probe():
    """f64 oracle and f32 oracle on the un-randomised model, every family: (state, M^-1 f64, b f64, M^-1 f32)"""
    n = 6
    cfg = load_env_cfg("bp5_imitation.yaml", num_envs=n)
    o64, o32 = O.OracleVecEnv(cfg), O.OracleVecEnv(cfg, precision="f32")
    out = {}
    for fam in DL.FAMILIES:
        st = DL.family_state(o64.get_state(), fam)
        o64.set_state(st); o32.set_state(st)
        out[fam] = (st, DL.oracle_probe(o64), DL.candidate_probe(o32)[0])
    return out


@pytest.mark.parametrize("fam", list(DL.FAMILIES))
def test_first_principles_over_the_families(fam, f64_probe):
    st, (minv, b), minv32 = f64_probe[fam]
    for i in range(st.shape[0]):
        gc = st[i, 0:19].copy()
        gc[3:7] /= np.linalg.norm(gc[3:7])                           # the f32-rounded quaternion is not exactly of unit length
        Mref = R.mass_matrix(gc)
        np.testing.assert_allclose(O.mass_matrix_world(gc), Mref, atol=2e-7)
        # M (independent numpy model) x M^-1 (f64 oracle env, read through its float32 getter) - I, against the f32 oracle's own residual
        res64, res32 = np.abs(Mref @ minv[i] - np.eye(18)).max(), np.abs(Mref @ minv32[i] - np.eye(18)).max()
        assert res64 <= 8.0 * res32, (fam, i, res64, res32)
        assert res32 < 1e-4                                           # ... which is itself at rounding level, so the line above binds
    rest = np.nonzero(~st[:, 19:37].any(axis=1))[0]
    assert len(rest) or fam in ("attitude", "one_hot_rate", "far_away")
    for i in rest[:2]:                                                 # at zero velocity the bias is the potential's gradient
        gc = st[i, 0:19].copy()
        gc[3:7] /= np.linalg.norm(gc[3:7])
        h = O.nonlinear_world(gc, np.zeros(18))
        assert h[2] == pytest.approx(8.88 * 9.81, abs=1e-9) and abs(h[0]) < 1e-9 and abs(h[1]) < 1e-9
        np.testing.assert_allclose(b[i], h, atol=2e-5)                 # the env's getter (float32 of values up to 90 N) is the same function
        eps = 1e-6
        for j in range(12):
            gp, gm = gc.copy(), gc.copy()
            gp[7 + j] += eps
            gm[7 + j] -= eps
            (cp, m), (cm, _) = R.com_world(gp), R.com_world(gm)
            assert h[6 + j] == pytest.approx(m * 9.81 * (cp[2] - cm[2]) / (2 * eps), abs=1e-6)


@pytest.mark.parametrize("n", [5, 24])
@pytest.mark.parametrize("emu", EMUS)
def test_emulated_kernel_source_probe_entrywise(emu, n):
    cfg = load_env_cfg(DL.PROBE_CFG, num_envs=n)
    orc, cand = O.OracleVecEnv(cfg), emu(cfg)
    for fam in DL.FAMILIES:
        st = DL.family_state(orc.get_state(), fam)
        orc.set_state(st); cand.set_state(st)
        DL.check_probe_entrywise(orc, cand, fam, label="emulation %d-lane n=%d" % (emu.WIDTH, n))


@pytest.mark.parametrize("n", [5, 24])
@pytest.mark.parametrize("emu", EMUS)
@pytest.mark.parametrize("pool", DL.POOLS, ids=DL.pool_id)
def test_emulated_kernel_source_substep_increment(pool, emu, n):
    DL.check_substep_increment(O.OracleVecEnv, emu, DL.pool_cfg(pool, n), pool[3], pool[1], label="emulation %d-lane n=%d %s" % (emu.WIDTH, n, DL.pool_id(pool)))
