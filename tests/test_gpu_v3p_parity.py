"""The 16-lane physics substep with pairs of 3-vectors on packed f32 instructions (csrc/env_core.hpp `v3p`): small pools through the flight
and the landing of a fresh reset, for the three kernel families the substep is compiled into.

Pools of 6 envs (one full wave of four robots and a wave with two live and two idle rows) and of 5, forced onto the 16-lane layout; 80 control
steps from reset under the benchmark's action stream (seed 1, sigma 0.3, the device generator): the robots hang 6 cm over the ground at reset, the
first toe touches after 26-32 steps and 32-42 of the 80 steps pass with no contact in the pool (the f64 oracle's count), so the wave-uniform contact
block is skipped in the first part and taken in the second.  For the flat pool (bp5_imitation.yaml,
kernels `shipped_flat`), the rough-ground pool (bp5_terrain.yaml, `shipped`) and the run-time-solver pool (ContactTolerance: 0, `md`):
  * ONE persistent launch of the 80 steps returns, row for row, what 80 one-step launches return, and leaves the same state -- bit for bit;
  * teacher-forced against the f64 oracle (parity_lib.check_teacher_forced with its own bounds, the ones test_gpu_parity.py runs under: TOL_STEP,
    events from 10x, cap 100x, budget 0.5 % -- which are also the TERRAIN_* constants of the rough-ground tests), every step taken BOTH as a one-step
    launch and as a persistent launch of one step on a second pool, which must agree bit for bit before the result is compared with the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import oracle as O
import parity_lib as PL
from conftest import load_env_cfg

K = 80
ACTION_SEED, ACTION_SIGMA = 1, 0.3      # bench.py's stream

POOLS = {"flat": ("bp5_imitation.yaml", {}, "shipped_flat", "irrl_steps_persistent_kernel_flat_l16"),
         "rough": ("bp5_terrain.yaml", {}, "shipped", "irrl_steps_persistent_kernel_l16"),
         "run_time_solver": ("bp5_imitation.yaml", {"ContactTolerance": 0.0}, "md", "irrl_steps_persistent_kernel_rt_l16")}


def _bench_table(n):
    from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib
    lib = _lib.load()
    table = torch.empty(K, n, 12, device="cuda")
    _lib.check(lib.irrl_bench_actions(ACTION_SEED, 0, n, 0, K, ACTION_SIGMA, C.c_void_p(table.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return table


def _outs(lead, n):
    return (torch.full(lead + (n, 35), float("nan"), device="cuda"), torch.full(lead + (n,), float("nan"), device="cuda"),
            torch.zeros(lead + (n,), dtype=torch.bool, device="cuda"), torch.full(lead + (n, 6), float("nan"), device="cuda"))


class _BothLaunches(object):
    """parity_lib candidate: every step() runs as a one-step launch on pool `a` and as a persistent launch of one step on pool `b`"""

    def __init__(self, a, b):
        self.a, self.b, self.n = a, b, a.n
        self.row = torch.empty(1, self.n, 12, device="cuda")
        self.out = _outs((1,), self.n)

    def set_state(self, st):
        self.a.set_state(st)
        self.b.set_state(st)

    def get_state(self):
        sa, sb = self.a.get_state(), self.b.get_state()
        np.testing.assert_array_equal(sa, sb)
        return sa

    def step(self, action):
        one = self.a.step(action)
        self.row[0].copy_(torch.from_numpy(np.ascontiguousarray(action, np.float32)))
        self.b.impl.step_rows(1, self.row, 0, *self.out, persistent=True)
        torch.cuda.synchronize()
        for what, x, y in zip(("ob", "reward", "done", "extraInfo"), one, self.out):
            assert np.array_equal(x, y[0].cpu().numpy()), "persistent launch of one step: %s differs from the one-step launch" % what
        return one


@pytest.mark.parametrize("n", [6, 5])
@pytest.mark.parametrize("pool", sorted(POOLS))
def test_paired_substep_persistent_rows_equal_one_step_launches_and_both_match_the_oracle(monkeypatch, pool, n):
    from hip_env import HipVecEnv
    monkeypatch.setenv("IRRL_LANES_PER_ROBOT", "16")
    name, over, variant, kernel = POOLS[pool]
    cfg = load_env_cfg(name, num_envs=n, **over)
    a, b = HipVecEnv(cfg), HipVecEnv(cfg)
    assert a.impl.lanes_per_robot == 16 and a.impl.kernel_variant == variant
    assert a.impl.persistent_supported == 1 and a.impl.kernel_name(1) == kernel
    table = _bench_table(n)
    # one launch of K steps against K launches of one step
    pers, want, one = _outs((K,), n), _outs((K,), n), _outs((), n)
    a.impl.step_rows(K, table, 0, *pers, persistent=True)
    for k in range(K):
        b.impl.step(table[k], *one)
        for w, o in zip(want, one):
            w[k].copy_(o)
    torch.cuda.synchronize()
    for what, p, w in zip(("ob", "reward", "done", "extraInfo"), pers, want):
        assert torch.equal(p, w), "%s: %s rows of the persistent launch differ from %d one-step launches" % (pool, what, K)
    np.testing.assert_array_equal(a.get_state(), b.get_state())
    contacts = a.get_state()[:, PL.S["INCONTACT"]:PL.S["INCONTACT"] + 4]
    assert contacts.any(), "no robot stands after %d steps: the contact path did not run" % K
    # both launch forms against the oracle, teacher-forced over the same 80 steps from reset
    rows = iter(table.cpu().numpy())
    monkeypatch.setattr(PL, "random_actions", lambda rng, n_envs, scale=0.3: next(rows))
    orc, cand = O.OracleVecEnv(cfg), _BothLaunches(HipVecEnv(cfg), HipVecEnv(cfg))
    airborne = []
    worst, _ = PL.check_teacher_forced(orc, cand, steps=K, after_step=lambda k, d_o, d_c: airborne.append(
        not orc.get_state()[:, PL.S["INCONTACT"]:PL.S["INCONTACT"] + 4].any()))
    print("[v3p %s, %d envs] steps with no contact in the pool: %d of %d; worst / tolerance: %s" % (pool, n, sum(airborne), K, worst["worst_factor"]))
    assert sum(airborne) >= 10 and K - sum(airborne) >= 10, "the 80 steps must hold a flight phase and a contact phase (%d airborne)" % sum(airborne)
