"""Entry-wise dynamics parity on a real MI355X: the HIP kernels through the C-ABI against the f64 oracle, at the bounds of
dynamics_parity_lib.BOUND (8 x the f32 oracle's own error) -- the probe on every state family, ragged pools bit for bit against a
pool of 48, and the velocity increment of one env step in free flight on every pool of dynamics_parity_lib.POOLS; every lane layout.
Each test prints its worst error / BOUND per block (DESIGN.md keeps the largest as a record)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as O
import dynamics_parity_lib as DL
from conftest import load_env_cfg

LAYOUTS = {"l16": (16, 1), "l4": (4, 1), "l4w2": (4, 2)}            # IRRL_LANES_PER_ROBOT, IRRL_L4_WAVES


def _hip(cfg):
    from hip_env import HipVecEnv
    return HipVecEnv(cfg)


def _hip_in_layout(layout, monkeypatch):
    lanes, waves = LAYOUTS[layout]
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", str(lanes))
    monkeypatch.setenv("IRRL_L4_WAVES", str(waves))

    def make(cfg):
        env = _hip(cfg)
        assert env.impl.lanes_per_robot == lanes and env.impl.waves_per_simd == waves, (env.impl.lanes_per_robot, env.impl.waves_per_simd)
        return env
    return make


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("family", list(DL.FAMILIES))
def test_probe_entrywise(family, layout, monkeypatch):
    cfg = load_env_cfg(DL.PROBE_CFG, num_envs=DL.N_REF)
    orc, cand = O.OracleVecEnv(cfg), _hip_in_layout(layout, monkeypatch)(cfg)
    st = DL.family_state(orc.get_state(), family)
    orc.set_state(st)
    cand.set_state(st)
    DL.check_probe_entrywise(orc, cand, family, label="MI355X %s" % layout)


_POOL_OF_48 = {}


def _probe_bits(make, n, family):
    cfg = load_env_cfg(DL.PROBE_CFG, num_envs=n)
    env = make(cfg)
    st = DL.family_state(env.get_state(), family)
    env.set_state(st)
    return st, env.probe()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("n", [1, 5, 37])
def test_ragged_pools_probe_the_same_bits_as_a_pool_of_48(n, layout, monkeypatch):
    """5 robots leave the last 16-lane wave a quarter full, 37 leave the last 4-lane wave ragged, 1 is the evaluation's pool: robot i's
    M^-1 and bias are those of robot i in a pool of 48, bit for bit."""
    make = _hip_in_layout(layout, monkeypatch)
    for family in ("nominal", "moving"):
        if (layout, family) not in _POOL_OF_48:
            _POOL_OF_48[layout, family] = _probe_bits(make, DL.N_REF, family)
        st48, (minv48, b48) = _POOL_OF_48[layout, family]
        st, (minv, b) = _probe_bits(make, n, family)
        assert np.array_equal(st, st48[:n])                                   # the same robots: pose, velocity and model parameters
        assert np.isfinite(minv).all() and np.abs(minv).max() > 50.0
        assert np.array_equal(minv, minv48[:n]), (family, np.nonzero((minv != minv48[:n]).any(1))[0])
        assert np.array_equal(b, b48[:n]), (family, np.nonzero((b != b48[:n]).any(1))[0])


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("pool", DL.POOLS, ids=DL.pool_id)
def test_substep_increment(pool, layout, monkeypatch):
    make = _hip_in_layout(layout, monkeypatch)
    cfg = DL.pool_cfg(pool, DL.N_INC)
    _, (cand, st, actions, after) = DL.check_substep_increment(O.OracleVecEnv, make, cfg, pool[3], pool[1], label="MI355X %s %s" % (layout, DL.pool_id(pool)))
    print("kernels: step %s, persistent %s" % (cand.impl.kernel_name(0), cand.impl.kernel_name(1)))
    if pool[2] == 8:
        # the same step as ONE persistent launch of K = 1 steps: the same pool state, bit for bit
        import torch
        other = make(cfg)
        other.set_state(st)
        n = other.n
        table = torch.from_numpy(np.ascontiguousarray(actions, np.float32)[None]).cuda()
        outs = (torch.zeros(1, n, 35, device="cuda"), torch.zeros(1, n, device="cuda"), torch.zeros(1, n, dtype=torch.bool, device="cuda"),
                torch.zeros(1, n, 6, device="cuda"))
        other.impl.step_rows(1, table, 0, *outs, persistent=True)
        torch.cuda.synchronize()
        assert not outs[2].any().item()
        assert np.array_equal(other.get_state(), after)
