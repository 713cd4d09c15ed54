"""Shared pieces of tests/test_ppo_loss_reference.py (CPU) and tests/test_gpu_ppo_loss_branches.py (MI355X): the branch table of the clipped
PPO2 loss, a builder that puts every sample of a batch into a CHOSEN branch, the coefficient sets, and the float64 reference of the five
kernels that carry the loss and its hand-written backward pass (irrl_ppo_loss, irrl_ppo_heads_loss, and the three MlpPolicy gradient kernels).

Reference = ppo2.ppo_loss + diag_gaussian_neglogp / diag_gaussian_entropy in float64 under torch autograd, the advantage statistics rounded to
float32 first (the kernels read them as floats).  Inputs are drawn ON THE CPU from a seed that is a function of the case, so the CPU module
checks the very tensors the GPU module feeds the kernels.  Errors are per tensor: max |out - f64| / max |f64| (lstm_forms_lib.rel_err).

The branch table, for cliprange c, ratio = exp(old_neglogp - neglogp), adv = (R - ov - a_mean) / (a_std + 1e-8), dv = v - ov:

  P1  adv > 0, ratio < 1 - c   active (gradient -adv), counts in clipfrac      V1  |dv| < c                 gradient v - R
  P2  adv > 0, ratio inside    active                                           V2  dv > c,  R above v       clipped out: EXACTLY 0
  P3  adv > 0, ratio > 1 + c   clipped out: EXACTLY 0, counts in clipfrac       V3  dv > c,  R below ov + c  active, v - R
  P4  adv < 0, ratio < 1 - c   clipped out: EXACTLY 0, counts in clipfrac       V4  dv < -c, R below v       clipped out: EXACTLY 0
  P5  adv < 0, ratio inside    active                                           V5  dv < -c, R above ov - c  active
  P6  adv < 0, ratio > 1 + c   active, counts in clipfrac
  P7  adv == 0.0 exactly, ratio outside: the pg1 == pg2 tie, gradient EXACTLY 0, counts in clipfrac

The policy class and the value class of a sample are coupled through s = R - ov (its sign against a_mean is the sign of adv; its position
against dv and +-c picks the value class), so only some pairs exist for a coefficient set: `feasible_pairs`.  P7 needs R - ov - a_mean == 0
in float32 AND in float64, which float32 inputs only give for a_mean == 0 with R == ov bit for bit: it is designed in the coefficient sets
whose a_mean is 0 and nowhere else.

Margins (conditions on the INPUTS, checked on the CPU): |ratio - (1 +- c)| >= 0.05, ||dv| - c| >= 0.05, |adv| >= 0.1 (not P7), |l1 - l2| >=
0.05 in V2 .. V5 -- neither f32 rounding nor the bf16x3 arithmetic (1e-4 relative on neglogp / v) can carry a sample across a boundary.
"""
import collections
import copy
import functools
import math

import numpy as np
import torch

from high_speed_quadrupedal_locomotion_by_irrl_amd import ppo2 as P2
from high_speed_quadrupedal_locomotion_by_irrl_amd.policies import MlpPolicy, diag_gaussian_entropy, diag_gaussian_neglogp
from lstm_forms_lib import fmt, rel_err  # noqa: F401  (the GPU module prints with them)

# the project's bounds for these arithmetics (test_fused_ppo_loss_matches_eager_graph, test_mlp_policy_gradient_kernels_match_autograd,
# test_fused_heads_and_loss_gradients_match_autograd): max |kernel - f64| / max |f64| per tensor
BOUNDS = {"loss_kernel": 2e-5, "heads": 2e-4, "f32": 2e-5, "bf16x3": 1e-4}
STATS_RTOL, STATS_ATOL, LOSS_TOL = 2e-4, 2e-5, 2e-5          # copies 1 - 2; the MLP forms: rtol = 10 tol, atol = tol, loss tol
STAT_NAMES = ("pg", "vf", "entropy", "approxkl", "clipfrac")

Coef = collections.namedtuple("Coef", "cliprange vf_coef ent_coef a_mean a_std")
# the last set is the second one at a_mean = 0: the narrow clip range with P7 rows in the mixed batches
COEF_SETS = [Coef(0.2, 0.5, 0.01, 0.0, 1.0), Coef(0.1, 1.0, 0.0, 0.3, 2.5), Coef(0.3, 0.25, 0.05, -0.4, 0.6), Coef(0.1, 1.0, 0.0, 0.0, 2.5)]

P_CLASSES, V_CLASSES = (1, 2, 3, 4, 5, 6, 7), (1, 2, 3, 4, 5)
P_ZERO, V_ZERO = (3, 4, 7), (2, 4)               # classes whose row gradient is exactly zero
P_OUTSIDE = (1, 3, 4, 6, 7)                      # classes that count in clipfrac
MARGIN = 0.05                                    # on the ratio, on |dv| and on |l1 - l2|
ADV_MARGIN = 0.1
# R - ov of an engineered sample lies in [S_LO, S_HI].  NOT symmetric: with a symmetric range the active rows' v - R cancel in the bias gradient of the
# value head -- ONE number, measured against itself -- to 1 / 2000 of its terms (467 samples, first coefficient set), and any f32 arithmetic, the eager
# graph included, is then 1e-5 .. 5e-5 off on it.  test_ppo_loss_reference.py holds the float32 eager graph to half of every f32 bound on every case.
S_LO, S_HI = -1.5, 2.5
PAD_ROWS = 70                                    # NaN rows behind a per-sample input, sentinel rows behind a per-row output
SENTINEL = 12345.0

LOSS_MS, LOSS_BLOCKS = (1, 63, 64, 65, 257, 1000), (1, 2, 2048)
HEADS_MS, HEADS_BLOCKS = (1, 63, 64, 65, 257, 700), (1, 2, 1024)
MLP_NS, MLP_BLOCKS = (1, 15, 16, 17, 197, 467), (1, 2, 256)
PURE_N = 48
# (name, ppo2.MLP_PRECISION, IRRL_MLP_WAVES, packed records)
MlpForm = collections.namedtuple("MlpForm", "name prec waves rec")
MLP_FORMS = [MlpForm("f32", "f32", "8", False), MlpForm("bf16x3-4waves", "bf16x3", "4", False), MlpForm("bf16x3-pairs", "bf16x3", "8", False),
             MlpForm("bf16x3-4waves-rec", "bf16x3", "4", True), MlpForm("bf16x3-pairs-rec", "bf16x3", "8", True)]
PURE_CLASSES = [("P", p) for p in P_CLASSES] + [("V", v) for v in V_CLASSES]


def class_id(pure):
    return "mixed" if pure is None else "%s%d" % pure


def seed_of(*key):
    s = 0
    for v in key:
        if isinstance(v, str):
            v = sum(ord(ch) for ch in v)
        s = (s * 1000003 + int(v) + 29) % (2 ** 31 - 1)
    return s


def adv_stats(coef):
    """(a_mean, a_std) as the float32 pair the kernels read"""
    return torch.tensor([coef.a_mean, coef.a_std], dtype=torch.float32)


# ---- which (policy class, value class) pairs a coefficient set admits, and the interval of s = R - ov of each ----
def feasible_pairs(coef):
    c = coef.cliprange
    a_mean, a_std = (float(x) for x in adv_stats(coef))
    t = 1.2 * ADV_MARGIN * (a_std + 1e-8)            # |s - a_mean| >= t  =>  |adv| >= 0.12
    pairs = collections.OrderedDict()
    for v in V_CLASSES:
        for p in P_CLASSES:
            lo, hi = S_LO, S_HI
            # dv = +-(c + u), u in [0.25, 0.5]; s at least 0.3 beyond v (V2, V4) or beyond ov +- c (V3, V5): |l1 - l2| = u (u + 2 w) >= 0.21
            if v == 2:
                lo = max(lo, c + 0.8)
            elif v == 3:
                hi = min(hi, c - 0.3)
            elif v == 4:
                hi = min(hi, -c - 0.8)
            elif v == 5:
                lo = max(lo, -c + 0.3)
            if p == 7:
                if a_mean != 0.0 or not (lo <= 0.0 <= hi):
                    continue
                lo = hi = 0.0
            else:
                if p <= 3:
                    lo = max(lo, a_mean + t)
                else:
                    hi = min(hi, a_mean - t)
                if hi - lo < 0.05:
                    continue
            pairs[(p, v)] = (lo, hi)
    return pairs


def design(M, coef, seed, pure=None):
    """The designed classes and targets of M samples: {pcls, vcls, ratio, dv, s} (numpy).  Mixed batches cycle through every feasible pair (in an
    order shuffled by the seed, beginning with a pair that is active in both terms, so that a batch of ONE sample has gradients); a pure batch
    through the pairs that contain the class `pure` = ("P", k) or ("V", k)."""
    rng = np.random.RandomState(seed)
    table = feasible_pairs(coef)
    keys = list(table)
    if pure is not None:
        keys = [k for k in keys if k[0 if pure[0] == "P" else 1] == pure[1]]
        assert keys, (coef, pure)
    else:
        first = (1, 5)
        assert first in table
        rest = [k for k in keys if k != first]
        keys = [first] + [rest[i] for i in rng.permutation(len(rest))]
    c = coef.cliprange
    pcls, vcls = np.zeros(M, np.int64), np.zeros(M, np.int64)
    ratio, dv, s = np.zeros(M), np.zeros(M), np.zeros(M)
    for i in range(M):
        p, v = keys[i % len(keys)]
        lo, hi = table[(p, v)]
        r1, r2, r3 = rng.uniform(), rng.uniform(), rng.uniform()
        pcls[i], vcls[i] = p, v
        s[i] = lo + r1 * (hi - lo)
        u = 0.25 + 0.25 * r2
        # V1: dv in [-0.25 w, w], both signs but not symmetric (a P7 row has R == ov, so its v - R IS dv: see S_LO, S_HI)
        dv[i] = (1.25 * r2 - 0.25) * (c - MARGIN - 0.01) if v == 1 else (c + u if v in (2, 3) else -c - u)
        pos = {1: 0, 4: 0, 2: 1, 5: 1, 3: 2, 6: 2}.get(p, 2 * ((i // len(keys)) % 2))       # P7: below and above in turn
        ratio[i] = (1.0 - c - MARGIN - 0.02 - 0.3 * r3, 1.0 + (2.0 * r3 - 1.0) * (c - MARGIN - 0.02), 1.0 + c + MARGIN + 0.02 + 0.5 * r3)[pos]
    return {"pcls": pcls, "vcls": vcls, "ratio": ratio, "dv": dv, "s": s}


def finish(des, nlp64, v64):
    """float32 old_neglogp, old_values, returns that put the float64 forward values (nlp64, v64) of the samples into the designed classes"""
    onlp = (nlp64.double() + torch.from_numpy(np.log(des["ratio"]))).float()
    ov = (v64.double() - torch.from_numpy(des["dv"])).float()
    R = (ov.double() + torch.from_numpy(des["s"])).float()       # s == 0 (P7): R == ov bit for bit
    return onlp, ov, R


def clipfrac_count(des):
    return int(np.isin(des["pcls"], P_OUTSIDE).sum())


def classify(nlp, v, R, ov, onlp, coef):
    """The class of every sample from forward values of any dtype (0 = in no class of the table), and the margins of the module docstring"""
    c = coef.cliprange
    st = adv_stats(coef).to(nlp.dtype)
    adv = (R - ov - st[0]) / (st[1] + 1e-8)
    ratio = torch.exp(onlp - nlp)
    pos = torch.where(ratio < 1.0 - c, 0, torch.where(ratio > 1.0 + c, 2, 1))
    pcls = torch.where(adv > 0, pos + 1, torch.where(adv < 0, pos + 4, torch.where(pos != 1, 7, 0)))
    dv = v - ov
    vcls = torch.where(dv.abs() < c, 1,
                       torch.where(dv > c, torch.where(R > v, 2, torch.where(R < ov + c, 3, 0)),
                                   torch.where(dv < -c, torch.where(R < v, 4, torch.where(R > ov - c, 5, 0)), 0)))
    vc = ov + torch.clamp(dv, -c, c)
    return {"pcls": pcls.numpy(), "vcls": vcls.numpy(), "adv": adv.double().numpy(), "ratio": ratio.double().numpy(),
            "ratio_margin": torch.minimum((ratio - (1.0 - c)).abs(), (ratio - (1.0 + c)).abs()).double().numpy(),
            "dv_margin": (dv.abs() - c).abs().double().numpy(), "l_margin": ((v - R) ** 2 - (vc - R) ** 2).abs().double().numpy()}


# ---- the reference ----
def loss_graph(mean, v, logstd, actions, R, ov, onlp, coef):
    """ppo2.ppo_loss on tensors of one dtype (float64: the reference; float32: the eager graph) -> loss, [pg, vf, entropy, approxkl, clipfrac]"""
    st = adv_stats(coef).to(mean.dtype)
    nadv = (R - ov - st[0]) / (st[1] + 1e-8)
    loss, pg, vf, ent, kl, cf = P2.ppo_loss(diag_gaussian_neglogp(actions, mean, logstd), v, diag_gaussian_entropy(logstd, mean), None, nadv, R, onlp, ov,
                                            coef.cliprange, coef.ent_coef, coef.vf_coef)
    return loss, torch.stack([pg, vf, ent, kl, cf])


def numpy_loss(mean, v, logstd, actions, R, ov, onlp, coef, pcls, vcls):
    """The loss written out in numpy float64, independent of ppo2.ppo_loss and of autograd: loss, statistics, and the row gradients
    d loss / d neglogp, d loss / d v from the branch table (an active policy row: adv ratio / M; an active value row: vf_coef (v - R) / M)."""
    M, A = actions.shape
    c = coef.cliprange
    a_mean, a_std = (float(x) for x in adv_stats(coef))
    nlp = 0.5 * (((actions - mean) / np.exp(logstd)) ** 2).sum(-1) + 0.5 * math.log(2.0 * math.pi) * A + logstd.sum()
    adv = (R - ov - a_mean) / (a_std + 1e-8)
    ratio = np.exp(onlp - nlp)
    pg = np.maximum(-adv * ratio, -adv * np.clip(ratio, 1.0 - c, 1.0 + c)).mean()
    vc = ov + np.clip(v - ov, -c, c)
    vf = 0.5 * np.maximum((v - R) ** 2, (vc - R) ** 2).mean()
    ent = float((logstd + 0.5 * (math.log(2.0 * math.pi) + 1.0)).sum())
    kl = 0.5 * ((nlp - onlp) ** 2).mean()
    cf = (np.abs(ratio - 1.0) > c).mean()
    loss = pg - coef.ent_coef * ent + coef.vf_coef * vf
    d_nlp = np.where(np.isin(pcls, P_ZERO), 0.0, adv * ratio / M)
    d_v = np.where(np.isin(vcls, V_ZERO), 0.0, coef.vf_coef * (v - R) / M)
    return loss, np.array([pg, vf, ent, kl, cf]), d_nlp, d_v


def padded(t, device="cpu", pad=PAD_ROWS, fill=float("nan")):
    """t as the leading slice of an allocation on `device` whose `pad` further rows hold `fill` (NaN behind an input, a sentinel behind an output):
    a kernel that reads or writes past the batch shows, and no address leaves the allocation.  The whole allocation is `._base` of the result."""
    big = torch.full((t.shape[0] + pad,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=device)
    big[:t.shape[0]].copy_(t)
    return big[:t.shape[0]]


def untouched_behind(view, fill=SENTINEL):
    """the rows behind a `padded` output still hold the sentinel"""
    tail = view._base[view.shape[0]:]
    return bool((tail == fill).all())


def _sign_convention_(w):
    # an orthogonal init comes out of an SVD, whose singular vectors are only defined up to a sign (lstm_forms_lib.make_seq_inputs): the largest
    # entry of every row is made positive, so that every machine draws the same weights
    big = w.gather(1, w.abs().argmax(1, keepdim=True))
    w.mul_(torch.where(big < 0, -1.0, 1.0))


# ---- copy 1: irrl_ppo_loss ----
LOSS_INPUTS = ("mean", "vpred", "actions", "returns", "old_values", "old_neglogp")


@functools.lru_cache(maxsize=None)
def make_loss_case(M, ci, pure=None):
    """-> {inputs (float32, CPU, never changed afterwards), "design", "ref": float64 loss, stats, d_mean, d_vpred, d_logstd}"""
    coef = COEF_SETS[ci]
    seed = seed_of("loss", M, ci, class_id(pure))
    g = torch.Generator().manual_seed(seed)
    mean, vpred = 0.5 * torch.randn(M, 12, generator=g), torch.randn(M, generator=g)
    logstd = 0.2 * torch.randn(1, 12, generator=g)
    actions = mean + torch.exp(logstd) * torch.randn(M, 12, generator=g)
    des = design(M, coef, seed, pure)
    m64, v64, ls64 = mean.double().requires_grad_(), vpred.double().requires_grad_(), logstd.double().requires_grad_()
    with torch.no_grad():
        onlp, ov, R = finish(des, diag_gaussian_neglogp(actions.double(), m64, ls64), v64)
    loss, stats = loss_graph(m64, v64, ls64, actions.double(), R.double(), ov.double(), onlp.double(), coef)
    gm, gv, gl = torch.autograd.grad(loss, [m64, v64, ls64])
    return {"M": M, "coef": coef, "design": des, "mean": mean, "vpred": vpred, "logstd": logstd, "actions": actions, "returns": R, "old_values": ov,
            "old_neglogp": onlp, "ref": {"loss": loss.detach(), "stats": stats.detach(), "d_mean": gm, "d_vpred": gv, "d_logstd": gl}}


def loss_forward(case, dtype):
    """neglogp and v of a copy-1 case in `dtype` (what `classify` takes)"""
    t = lambda k: case[k].to(dtype)
    return diag_gaussian_neglogp(t("actions"), t("mean"), t("logstd")), t("vpred")


def loss_eager_f32(case):
    """the float32 eager graph of a copy-1 case -> {d_mean, d_vpred, d_logstd}: what a fallback bound is four times the error of"""
    m, v, ls = (case[k].clone().requires_grad_() for k in ("mean", "vpred", "logstd"))
    loss, _ = loss_graph(m, v, ls, case["actions"], case["returns"], case["old_values"], case["old_neglogp"], case["coef"])
    return dict(zip(("d_mean", "d_vpred", "d_logstd"), torch.autograd.grad(loss, [m, v, ls])))


# ---- copy 2: irrl_ppo_heads_loss ----
HEADS_INPUTS = ("h_pi", "h_v", "actions", "returns", "old_values", "old_neglogp")
HEADS_WEIGHTS = ("pi_w", "pi_b", "vf_w", "vf_b", "logstd")
HEADS_GRADS = ("d_hpi", "d_hv", "d_wpi", "d_bpi", "d_wv", "d_bv", "d_logstd")


def heads_forward(case, dtype):
    t = lambda k: case[k].to(dtype)
    mean = t("h_pi") @ t("pi_w") + t("pi_b")
    return diag_gaussian_neglogp(t("actions"), mean, t("logstd")), (t("h_v") @ t("vf_w") + t("vf_b")).squeeze(-1)


@functools.lru_cache(maxsize=None)
def make_heads_case(M, ci, pure=None):
    """random latents |h| < 1, heads of the scale test_fused_heads_and_loss_gradients_match_autograd uses -> inputs, design, float64 reference
    (also the heads' own outputs "mean", "value")"""
    coef = COEF_SETS[ci]
    seed = seed_of("heads", M, ci, class_id(pure))
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    case = {"M": M, "coef": coef, "h_pi": 1.998 * torch.rand(M, 48, generator=g) - 0.999, "h_v": 1.998 * torch.rand(M, 48, generator=g) - 0.999,
            "pi_w": 0.2 * rn(48, 12), "pi_b": 0.1 * rn(12), "vf_w": 0.2 * rn(48, 1), "vf_b": 0.1 * rn(1), "logstd": 0.2 * rn(1, 12), "actions": 0.7 * rn(M, 12)}
    des = design(M, coef, seed, pure)
    leaves = [case[k].double().requires_grad_() for k in ("h_pi", "h_v") + HEADS_WEIGHTS]
    hp, hv, pw, pb, vw, vb, ls = leaves
    mean, v = hp @ pw + pb, (hv @ vw + vb).squeeze(-1)
    with torch.no_grad():
        onlp, ov, R = finish(des, diag_gaussian_neglogp(case["actions"].double(), mean, ls), v)
    loss, stats = loss_graph(mean, v, ls, case["actions"].double(), R.double(), ov.double(), onlp.double(), coef)
    grads = torch.autograd.grad(loss, leaves)
    ref = dict(zip(HEADS_GRADS, grads))
    ref.update(loss=loss.detach(), stats=stats.detach(), mean=mean.detach(), value=v.detach())
    case.update(design=des, returns=R, old_values=ov, old_neglogp=onlp, ref=ref)
    return case


def heads_eager_f32(case):
    """the float32 eager graph of a copy-2 case -> {name: gradient} over HEADS_GRADS"""
    leaves = [case[k].clone().requires_grad_() for k in ("h_pi", "h_v") + HEADS_WEIGHTS]
    hp, hv, pw, pb, vw, vb, ls = leaves
    loss, _ = loss_graph(hp @ pw + pb, (hv @ vw + vb).squeeze(-1), ls, case["actions"], case["returns"], case["old_values"], case["old_neglogp"], case["coef"])
    return dict(zip(HEADS_GRADS, torch.autograd.grad(loss, leaves)))


# ---- copies 3 - 5: the MlpPolicy gradient kernels ----
MLP_INPUTS = ("obs", "actions", "returns", "old_values", "old_neglogp")


def mlp_params(pol):
    """the 13 parameters the gradient kernels differentiate (the unused q head has no gradient), stable-baselines order"""
    return [q for q in pol.sb_parameters() if q is not pol.q.w and q is not pol.q.b]


MLP_PARAM_NAMES = ("pi_fc0.w", "pi_fc0.b", "vf_fc0.w", "vf_fc0.b", "pi_fc1.w", "pi_fc1.b", "vf_fc1.w", "vf_fc1.b", "vf.w", "vf.b", "pi.w", "pi.b", "logstd")
MLP_POLICY_NET = ("pi_fc0.w", "pi_fc0.b", "pi_fc1.w", "pi_fc1.b", "pi.w", "pi.b")      # + logstd, whose gradient also carries -ent_coef
MLP_VALUE_NET = ("vf_fc0.w", "vf_fc0.b", "vf_fc1.w", "vf_fc1.b", "vf.w", "vf.b")


@functools.lru_cache(maxsize=None)
def make_mlp_policy(seed):
    """MlpPolicy away from its symmetric initial point, as test_mlp_policy_gradient_kernels_match_autograd moves it (float32, CPU; copy before use)"""
    torch.manual_seed(seed)
    pol = MlpPolicy()
    g = torch.Generator().manual_seed(seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g)
    with torch.no_grad():
        for l in (*pol.pi_fc, *pol.vf_fc, pol.pi, pol.vf):
            _sign_convention_(l.w)
        pol.pi.w.mul_(30.0)
        pol.pi.b.add_(0.1 * rn(12))
        pol.logstd.add_(0.2 * rn(1, 12))
        pol.vf.b.add_(0.1 * rn(1))
        for l in (*pol.pi_fc, *pol.vf_fc):
            l.b.add_(0.1 * rn(*l.b.shape))
    return pol


def mlp_forward(case, dtype):
    pol = copy.deepcopy(case["policy"]).to(dtype)
    sel = case["rows"]
    with torch.no_grad():
        mean, v = pol._run(case["obs"][sel].to(dtype))
        return diag_gaussian_neglogp(case["actions"][sel].to(dtype), mean, pol.logstd), v


@functools.lru_cache(maxsize=None)
def make_mlp_case(n, indexed, ci, pure=None):
    """-> {"policy", the five flat arrays (float32; every row the minibatch does not use holds NaN), "index" (int64 [n] or None), "rows" (the rows
    in the minibatch's order), design, "ref": float64 loss, stats, grads {name: gradient}}.  indexed: a shuffled index into 2 n + 77 rows;
    otherwise rows 0 .. n-1 of n + PAD_ROWS."""
    coef = COEF_SETS[ci]
    seed = seed_of("mlp", n, int(indexed), ci, class_id(pure))
    pol = make_mlp_policy(seed_of("mlp-policy", n))
    g = torch.Generator().manual_seed(seed)
    total = 2 * n + 77 if indexed else n + PAD_ROWS
    rows = torch.randperm(total, generator=g)[:n].contiguous() if indexed else torch.arange(n)
    obs, actions = torch.randn(n, 35, generator=g), 0.5 * torch.randn(n, 12, generator=g)
    des = design(n, coef, seed, pure)
    p64 = copy.deepcopy(pol).double()
    mean, v = p64._run(obs.double())
    with torch.no_grad():
        onlp, ov, R = finish(des, diag_gaussian_neglogp(actions.double(), mean, p64.logstd), v)
    loss, stats = loss_graph(mean, v, p64.logstd, actions.double(), R.double(), ov.double(), onlp.double(), coef)
    grads = torch.autograd.grad(loss, mlp_params(p64))
    case = {"n": n, "coef": coef, "policy": pol, "index": rows if indexed else None, "rows": rows, "design": des,
            "ref": {"loss": loss.detach(), "stats": stats.detach(), "grads": dict(zip(MLP_PARAM_NAMES, grads))}}
    for name, t in zip(MLP_INPUTS, (obs, actions, R, ov, onlp)):
        full = torch.full((total,) + tuple(t.shape[1:]), float("nan"))
        full[rows] = t
        case[name] = full
    return case


# ---- float64 model of the bf16x3 arithmetic of the MlpPolicy kernels: every matrix-product operand as hi = bf16(v), lo = bf16(v - hi), a product
#      as hi hi + hi lo + lo hi summed in float64 (lstm_forms_lib._Split3MatMul); everything else exact ----
def mlp_bf16x3_model(case):
    """-> loss, stats, {name: gradient} of the case under the two-plane model (the fallback bound of a bf16x3 form is 4 x its error)"""
    from lstm_forms_lib import _Split3MatMul
    mm = _Split3MatMul.apply
    p64 = copy.deepcopy(case["policy"]).double()
    sel = case["rows"]
    d = lambda k: case[k][sel].double()

    def net(fc, head, x):
        for l in fc:
            x = torch.tanh(mm(x, l.w) + l.b)
        return mm(x, head.w) + head.b
    mean, v = net(p64.pi_fc, p64.pi, d("obs")), net(p64.vf_fc, p64.vf, d("obs")).squeeze(-1)
    loss, stats = loss_graph(mean, v, p64.logstd, d("actions"), d("returns"), d("old_values"), d("old_neglogp"), case["coef"])
    grads = torch.autograd.grad(loss, mlp_params(p64))
    return loss.detach(), stats.detach(), dict(zip(MLP_PARAM_NAMES, grads))


def mlp_eager_f32(case):
    """the float32 eager graph (ppo_loss on the eager policy) on the case's rows -> loss, stats, {name: gradient}: the fallback bound of the f32 form"""
    pol = copy.deepcopy(case["policy"])
    sel = case["rows"]
    f = lambda k: case[k][sel]
    coef = case["coef"]
    st = adv_stats(coef)
    mean, v = pol._run(f("obs"))
    nadv = (f("returns") - f("old_values") - st[0]) / (st[1] + 1e-8)
    loss, pg, vf, ent, kl, cf = P2.ppo_loss(diag_gaussian_neglogp(f("actions"), mean, pol.logstd), v, diag_gaussian_entropy(pol.logstd, mean), None, nadv,
                                            f("returns"), f("old_neglogp"), f("old_values"), coef.cliprange, coef.ent_coef, coef.vf_coef)
    grads = torch.autograd.grad(loss, mlp_params(pol))
    return loss.detach(), torch.stack([pg, vf, ent, kl, cf]).detach(), dict(zip(MLP_PARAM_NAMES, grads))
