"""The Python layer between the learner and the C-ABI (_lib marshalling helpers, the shared pieces of the four rollout wrappers in
lstm_fused, the MlpPolicy partial-sum layout and scatter map of ppo2): CPU tests of the argument decoding, GPU tests that every
accepted argument form gives the same bits and that the rollout wrappers equal the stepwise loop."""
import gc
import os
import re

import numpy as np
import pytest
import torch

from high_speed_quadrupedal_locomotion_by_irrl_amd import _lib, lstm_fused
from high_speed_quadrupedal_locomotion_by_irrl_amd import ppo2 as P2
from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import CustomLSTMPolicy, MlpPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "high_speed_quadrupedal_locomotion_by_irrl_amd", "csrc", "mlp_update.hpp")


def _header_constants():
    """every `#define IRRL_MLP_<name> <integer expression>` of csrc/mlp_update.hpp, evaluated"""
    out = {}
    for name, expr in re.findall(r"^#define\s+(IRRL_MLP_\w+)\s+([0-9+* ()]+?)\s*$", open(HEADER).read(), re.M):
        out[name] = int(eval(expr, {"__builtins__": {}}))
    return out


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_mlp_partial_layout_is_the_headers():
    c = _header_constants()
    names = {"dlogstd": "IRRL_MLP_P_DLS", "db1": "IRRL_MLP_P_DB1", "db2": "IRRL_MLP_P_DB2", "db3": "IRRL_MLP_P_DB3",
             "dW1": "IRRL_MLP_P_DW1", "dW2": "IRRL_MLP_P_DW2", "dW3": "IRRL_MLP_P_DW3"}
    lay = P2.MLP_PARTIAL_LAYOUT
    assert set(lay) == set(names) | {"scalars"}
    assert lay["scalars"][0] == 0
    for name, macro in names.items():
        assert lay[name][0] == c[macro], (name, lay[name], c[macro])
    assert P2.MLP_PARTIAL_LEN == c["IRRL_MLP_P"]
    # the pieces tile [0, IRRL_MLP_P): no gap, no overlap
    covered = np.zeros(c["IRRL_MLP_P"], np.int32)
    for o, r, k in lay.values():
        assert 0 <= o and o + r * k <= c["IRRL_MLP_P"]
        covered[o:o + r * k] += 1
    assert (covered == 1).all()
    # the padded shapes of the kernels: 48 input rows for IRRL_MLP_OB observations, 16 head columns
    assert lay["dW1"][1:] == (48, c["IRRL_MLP_H"]) and lay["dW2"][1:] == (c["IRRL_MLP_H"],) * 2 and lay["dW3"][1:] == (c["IRRL_MLP_H"], 16)
    assert c["IRRL_MLP_OB"] <= 48
    # a packed sample record: what mlp_pack_records allocates per sample (and its 256-byte alignment assertion)
    assert c["IRRL_MLP_REC"] == 64 == P2.MLP_RECORD_FLOATS and P2.MLP_RECORD_FLOATS * 4 == 256


def test_mlp_scatter_map_follows_the_header_offsets():
    """`_mlp_scatter_map` built from the layout table against the map written out from the header's offsets by hand"""
    c = _header_constants()
    pol = MlpPolicy()
    flat = P2.FlatParams(pol)
    mp, add = (t.numpy() for t in P2._mlp_scatter_map(pol, flat, 0.01))
    P, A = c["IRRL_MLP_P"], pol.act_dim
    want, want_add = np.full((2, P), -1, np.int32), np.zeros((2, P), np.float32)
    off = flat.offset_of
    for kind, fc, head in ((0, pol.pi_fc, pol.pi), (1, pol.vf_fc, pol.vf)):
        out = head.w.shape[1]
        want[kind, 0:4] = flat.n + 4 * kind + np.arange(4)
        want[kind, c["IRRL_MLP_P_DB1"]:c["IRRL_MLP_P_DB1"] + 64] = off[id(fc[0].b)] + np.arange(64)
        want[kind, c["IRRL_MLP_P_DB2"]:c["IRRL_MLP_P_DB2"] + 64] = off[id(fc[1].b)] + np.arange(64)
        want[kind, c["IRRL_MLP_P_DB3"]:c["IRRL_MLP_P_DB3"] + out] = off[id(head.b)] + np.arange(out)
        want[kind, c["IRRL_MLP_P_DW1"]:c["IRRL_MLP_P_DW1"] + 35 * 64] = off[id(fc[0].w)] + np.arange(35 * 64)
        want[kind, c["IRRL_MLP_P_DW2"]:c["IRRL_MLP_P_DW2"] + 64 * 64] = off[id(fc[1].w)] + np.arange(64 * 64)
        for i in range(64):
            want[kind, c["IRRL_MLP_P_DW3"] + 16 * i:c["IRRL_MLP_P_DW3"] + 16 * i + out] = off[id(head.w)] + i * out + np.arange(out)
    want[0, c["IRRL_MLP_P_DLS"]:c["IRRL_MLP_P_DLS"] + A] = off[id(pol.logstd)] + np.arange(A)
    want_add[0, c["IRRL_MLP_P_DLS"]:c["IRRL_MLP_P_DLS"] + A] = -0.01
    assert mp.dtype == np.int32 and np.array_equal(mp, want)
    assert add.dtype == np.float32 and np.array_equal(add, want_add)
    # every parameter slot the kernels produce a gradient for is written exactly once; `q` (no gradient) is not
    slots = mp[mp >= 0]
    assert len(np.unique(slots)) == len(slots)
    assert not np.isin(off[id(pol.q.w)] + np.arange(pol.q.w.numel()), slots).any()


def test_scatter_maps_belong_to_their_flat_params():
    pols = [MlpPolicy() for _ in range(3)]
    f1, f2 = P2.FlatParams(pols[0]), P2.FlatParams(pols[1])
    m1, m2 = P2._mlp_scatter_map(pols[0], f1, 0.01), P2._mlp_scatter_map(pols[1], f2, 0.01)
    assert all(a is not b for a in m1 for b in m2)
    assert all(a is b for a, b in zip(m1, P2._mlp_scatter_map(pols[0], f1, 0.01)))          # built once per (flat, ent_coef)
    other = P2._mlp_scatter_map(pols[0], f1, 0.02)
    assert other[0] is not m1[0] and float(other[1].min()) == np.float32(-0.02) and float(m1[1].min()) == np.float32(-0.01)
    assert all(a is b for a, b in zip(m1, P2._mlp_scatter_map(pols[0], f1, 0.01)))          # ... and the first one is still there
    # a learner that comes into being after the first one is gone never sees the first one's map, wherever it is allocated
    dead = list(m1) + list(other)
    del f1, m1, other
    pols[0] = None
    gc.collect()
    for _ in range(4):
        f3 = P2.FlatParams(pols[2])
        m3 = P2._mlp_scatter_map(pols[2], f3, 0.01)
        assert all(a is not b for a in m3 for b in dead) and all(a is not b for a in m3 for b in m2)
        assert torch.equal(m3[0], m2[0]) and torch.equal(m3[1], m2[1])                      # same architecture, same slots
        assert f3.mlp_maps[0.01] is m3
        del f3, m3
        gc.collect()


def test_ptr_and_contig():
    assert _lib.ptr(None) is None
    t = torch.arange(12.0).reshape(3, 4)
    assert _lib.ptr(t).value == t.data_ptr()
    assert _lib.ptr(t[1:]).value == t.data_ptr() + 16
    assert _lib.contig(t) is t
    u = _lib.contig(t.t())
    assert u.is_contiguous() and torch.equal(u, t.t())


def test_check_rc_names_the_entry_point_and_the_dimensions():
    _lib.check_rc(0, "irrl_sum_rows", rows=3)
    with pytest.raises(RuntimeError) as e:
        _lib.check_rc(1, "irrl_lstm_seq_forward_x", hid=48, T=5, N=40)
    assert str(e.value) == "irrl_lstm_seq_forward_x failed (rc=1, hid=48, T=5, N=40)"


def test_sampling_arguments_decode():
    dec = lstm_fused._sampling_args
    short = dec(None, (5, 9))
    assert short == (None, 1, 5, 9, None, 0)
    assert dec(None, (5, 9, None)) == short and dec(None, (5, 9, None, 0)) == short
    assert dec(None, (5, 9, None, 4096)) == (None, 1, 5, 9, None, 4096)                     # a 4-tuple carries env0
    assert dec(None, ((7 << 32) + 5, 9))[2] == 5 and dec(None, (-1, 9))[2] == 0xFFFFFFFF      # the seed is masked to 32 bits
    assert dec(None, (5, (5 << 32) + 42))[3] == (5 << 32) + 42                               # the step is 64 bits wide
    base = torch.zeros(1, dtype=torch.long)
    got = dec(None, (5, 9, base, 3))
    assert got[:4] == (None, 1, 5, 9) and got[4].value == base.data_ptr() and got[5] == 3
    # a given noise switches the kernel RNG off, whatever rng says
    noise = torch.zeros(4, 12)
    for rng in (None, (5, 9), (5, 9, base, 3)):
        got = dec(noise, rng)
        assert got[0].value == noise.data_ptr() and got[1:] == (0, 0, 0, None, 0)
    assert dec(None, None) == (None, 0, 0, 0, None, 0)                                       # deterministic


def _cpu_rollout_dict(T=3, N=5, **drop):
    d = dict(row=1, mb_obs=torch.zeros(T, N, 35), mb_actions=torch.zeros(T, N, 12), mb_values=torch.zeros(T, N), mb_neglogpacs=torch.zeros(T, N),
             mb_dones=torch.zeros(T, N, dtype=torch.bool), mb_rewards=torch.zeros(T, N), prev_reward=torch.zeros(N))
    return {k: v for k, v in d.items() if k not in drop}


def test_rollout_buffer_pointers():
    assert lstm_fused._step_buffer_ptrs(None) == (-1, [None] * 7)
    full = _cpu_rollout_dict()
    order = ("mb_obs", "mb_actions", "mb_values", "mb_neglogpacs", "mb_dones", "mb_rewards", "prev_reward")
    row, ptrs = lstm_fused._step_buffer_ptrs(full)
    assert row == 1 and [p.value for p in ptrs] == [full[k].data_ptr() for k in order]
    part = _cpu_rollout_dict(mb_rewards=1, prev_reward=1)
    row, ptrs = lstm_fused._step_buffer_ptrs(part)
    assert row == 1 and [p.value for p in ptrs[:5]] == [part[k].data_ptr() for k in order[:5]] and ptrs[5:] == [None, None]
    with pytest.raises(KeyError):
        lstm_fused._step_buffer_ptrs(_cpu_rollout_dict(mb_values=1))
    # the rollout form: all six buffers, then the env's reward and extra rows
    rew, extra = torch.zeros(5), torch.zeros(5, 6)
    row, ptrs = lstm_fused._rollout_buffer_ptrs(full, rew, extra)
    assert row == 1 and [p.value for p in ptrs] == [full[k].data_ptr() for k in order[:6]] + [rew.data_ptr(), extra.data_ptr()]
    for k in order[:6]:
        with pytest.raises(KeyError):
            lstm_fused._rollout_buffer_ptrs(_cpu_rollout_dict(**{k: 1}), rew, extra)
        with pytest.raises(KeyError):
            lstm_fused._rollout_buffer_ptrs(dict(full, **{k: None}), rew, extra)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _policy(kind, dev, seed):
    torch.manual_seed(seed)
    pol = (CustomLSTMPolicy(n_lstm=(48, 48)) if kind == "lstm" else MlpPolicy()).to(dev)
    with torch.no_grad():
        for p in pol.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    if hasattr(pol, "prepare"):
        pol.prepare()
    return pol


def _buffers(T, N, dev):
    return dict(mb_obs=torch.zeros(T, N, 35, device=dev), mb_actions=torch.zeros(T, N, 12, device=dev), mb_values=torch.zeros(T, N, device=dev),
                mb_neglogpacs=torch.zeros(T, N, device=dev), mb_dones=torch.zeros(T, N, dtype=torch.bool, device=dev),
                mb_rewards=torch.zeros(T, N, device=dev))


def _step(kind, pol, obs, st, dones, **kw):
    """-> (action, clipped, value, neglogp[, states_out]) through the module-level wrappers"""
    if kind == "lstm":
        return lstm_fused.policy_step(pol, obs, st, dones, **kw)
    return lstm_fused.mlp_policy_step(pol, obs, dones, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [7, 40])          # fewer robots than one 16-row tile; a full tile and a ragged last one
@pytest.mark.parametrize("kind", ["lstm", "mlp"])
def test_argument_forms_give_the_same_bits(kind, N):
    dev = torch.device("cuda")
    pol = _policy(kind, dev, 100 + N)
    obs = torch.randn(N, 35, device=dev)
    st = torch.randn(N, 384, device=dev) * 0.5 if kind == "lstm" else None
    dones = torch.rand(N, device=dev) < 0.2
    zero = torch.zeros(1, dtype=torch.long, device=dev)
    s, t = 1234567, (3 << 32) + 17
    # the three spellings of "no base, env 0"
    ref = [x.clone() for x in _step(kind, pol, obs, st, dones, rng=(s, t))]
    assert not torch.equal(ref[0], _step(kind, pol, obs, st, dones)[0])                      # (the RNG is on)
    for rng in ((s, t, zero), (s, t, zero, 0), (s, t, None), (s, t, None, 0)):
        got = _step(kind, pol, obs, st, dones, rng=rng)
        assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref)), rng
    # a given noise: rng is not looked at
    noise = torch.randn(N, 12, device=dev)
    ref = [x.clone() for x in _step(kind, pol, obs, st, dones, noise=noise)]
    assert not torch.equal(ref[0], _step(kind, pol, obs, st, dones, rng=(s, t))[0])
    for rng in ((s, t), (s, t, zero, 5)):
        got = _step(kind, pol, obs, st, dones, noise=noise, rng=rng)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), rng
    # rollout rows: leaving mb_rewards / prev_reward out leaves the other five rows as they are (and the outputs)
    full, part = _buffers(3, N, dev), _buffers(3, N, dev)
    prev = torch.randn(N, device=dev)
    a = _step(kind, pol, obs, st, dones, noise=noise, rollout=dict(full, row=1, prev_reward=prev))
    b = _step(kind, pol, obs, st, dones, noise=noise, rollout=dict({k: v for k, v in part.items() if k != "mb_rewards"}, row=1))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(torch.equal(x, y) for x, y in zip(a, ref))
    for k in ("mb_obs", "mb_actions", "mb_values", "mb_neglogpacs", "mb_dones"):
        assert torch.equal(full[k], part[k]), k
        assert full[k][1].any() or k == "mb_dones"
    assert torch.equal(full["mb_obs"][1], obs) and torch.equal(full["mb_actions"][1], a[0]) and torch.equal(full["mb_dones"][1], dones)
    assert torch.equal(full["mb_rewards"][0], prev) and not full["mb_rewards"][1:].any() and not part["mb_rewards"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lstm", "mlp"])
def test_rollout_wrappers_equal_the_stepwise_loop(kind):
    """`policy_rollout` / `mlp_policy_rollout` (one C call; two launches per step and ONE persistent launch) against T x (fused_step +
    env.step_into) from the same snapshot of the pool: 40 robots = a full and a ragged 16-robot workgroup, 3 steps = a first, a middle and
    a last reward row (rewards are written one row behind).  Everything bit for bit."""
    import yaml
    import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg
    from conftest import load_env_cfg
    from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv
    from high_speed_quadrupedal_locomotion_by_irrl_amd.vec_env import TorchVecEnv
    N, T = 40, 3
    dev = torch.device("cuda")
    env = TorchVecEnv(FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, yaml.safe_dump(load_env_cfg("default_cfg.yaml", num_envs=N))))
    pol = _policy(kind, dev, 7)
    lib = _lib.load()
    supports = lib.irrl_lstm_rollout_supports if kind == "lstm" else lib.irrl_mlp_rollout_supports
    assert supports(env.wrapper._h, 48 if kind == "lstm" else 64, 2) == 1          # fused=2 below IS the persistent kernel, not its fallback
    obs0 = env.reset().clone()
    env.wrapper.snapshot()
    st0 = torch.randn(N, 384, device=dev) * 0.5
    dones0 = torch.zeros(N, dtype=torch.bool, device=dev)
    dones0[3] = dones0[37] = True
    base = torch.tensor([11], dtype=torch.long, device=dev)
    seed = 4242

    def start():
        env.wrapper.restore()
        out = (torch.empty(N, 12, device=dev), torch.empty(N, 12, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev))
        return dict(obs=obs0.clone(), states=st0.clone(), dones=dones0.clone(), rew=torch.zeros(N, device=dev), **_buffers(T, N, dev)), out

    def frozen(s):
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in s.items()}          # every mb_* buffer, obs, dones, states and the last reward

    s, out = start()
    for t in range(T):
        clipped = pol.fused_step(s["obs"], s["states"] if kind == "lstm" else None, s["dones"], rng=(seed, t, base, 0), states_out=s["states"], out=out,
                                 rollout=dict(row=t, prev_reward=s["rew"], **{k: s[k] for k in s if k.startswith("mb_")}))[1]
        env.step_into(clipped, s["obs"], s["rew"], s["dones"])
    want = frozen(s)
    assert not torch.equal(want["obs"], obs0) and want["mb_rewards"][:T - 1].any() and not want["mb_rewards"][T - 1].any()
    for fused in (0, 2):
        s, out = start()
        rollout = dict(row=0, **{k: s[k] for k in s if k.startswith("mb_")})
        args = (s["dones"], (seed, 0, base, 0), rollout, out, s["rew"], env.extra)
        if kind == "lstm":
            lstm_fused.policy_rollout(pol, env.wrapper, T, s["obs"], s["states"], *args, fused=fused)
        else:
            lstm_fused.mlp_policy_rollout(pol, env.wrapper, T, s["obs"], *args, fused=fused)
        got = frozen(s)
        for k in want:
            assert torch.equal(got[k], want[k]), (kind, fused, k)
