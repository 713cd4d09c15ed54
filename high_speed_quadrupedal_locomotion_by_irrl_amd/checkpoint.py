"""Checkpoint interchange with the reference.

  read_checkpoint(path)        this build's pickles AND stable-baselines 2.8 pickles such as the reference's
                               IRRL/script/pkl/bp5_155.pkl: `(data dict, [19 np arrays])` written by
                               PPO2.save -> _save_to_file(cloudpickle=True) (ppo2.py:452-476).  The SB pickle
                               embeds tensorflow / gym / cloudpickle objects; a stub unpickler replaces them so
                               neither package is needed (only the hyper-parameters and the arrays are kept).
  export_actor_csv(model, dir) the reference's `--o` export (CustomerLstmNN.save_model, NN:203-224):
                               lstm_wx{i}.csv, lstm_wh{i}.csv, lstm_b{i}.csv, pi_w.csv, pi_b.csv with '%.6f'.
  NumpyLstmActor               numpy float64 twin of CustomerLstmNN.predict (NN:112-135), one vector or a batch with per-row resets:
                               the one numpy actor of the deployment checks and of every host-side evaluation loop.
"""
import os
import pickle

import numpy as np


class _Stub(object):
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Stub()

    def __setstate__(self, s):
        self.state = s

    def __getattr__(self, n):
        if n.startswith("__"):
            raise AttributeError(n)
        return _Stub()


def _stub_fn(*a, **k):
    return _Stub()


class _StubUnpickler(pickle.Unpickler):
    """ALLOW-LIST unpickler: a checkpoint only ever needs numpy arrays, plain containers and scalars.  Exactly the globals
    below resolve to the real thing; every other global a pickle names -- the tensorflow / gym / cloudpickle / stable_baselines
    objects of a reference checkpoint, but also `os.system`, `builtins.eval` or anything else a crafted file could ask for --
    becomes an inert stub that ignores its arguments.  Loading a checkpoint can therefore not run foreign code."""
    _ALLOWED = {
        ("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct"), ("numpy.core.multiarray", "scalar"),
        ("numpy._core.multiarray", "scalar"), ("numpy", "ndarray"), ("numpy", "dtype"), ("numpy.core.numeric", "_frombuffer"),
        ("numpy._core.numeric", "_frombuffer"), ("numpy", "float32"), ("numpy", "float64"), ("numpy", "int32"), ("numpy", "int64"), ("numpy", "bool_"),
        ("collections", "OrderedDict"), ("_codecs", "encode"),
        ("builtins", "list"), ("builtins", "dict"), ("builtins", "tuple"), ("builtins", "set"), ("builtins", "frozenset"), ("builtins", "int"),
        ("builtins", "float"), ("builtins", "bool"), ("builtins", "str"), ("builtins", "bytes"), ("builtins", "bytearray"), ("builtins", "complex"),
        ("builtins", "slice"), ("builtins", "range"), ("__builtin__", "list"), ("__builtin__", "dict"), ("__builtin__", "tuple"), ("__builtin__", "set"),
    }
    _FNS = ("CodeType", "code", "_make_skel_func", "_fill_function", "_builtin_type", "_make_cell", "_make_empty_cell",
            "_rehydrate_skeleton_class", "_make_skeleton_class", "subimport")

    def find_class(self, module, name):
        if (module, name) in self._ALLOWED:
            return super().find_class(module, name)
        return _stub_fn if name in self._FNS else _Stub


def read_checkpoint(path):
    if not os.path.exists(path) and os.path.exists(path + ".pkl"):
        path = path + ".pkl"
    with open(path, "rb") as f:
        data, params = _StubUnpickler(f).load()
    if isinstance(params, dict):
        params = list(params.values())
    clean = {}
    for k, v in dict(data).items():
        clean[k] = v if isinstance(v, (int, float, str, list, dict, tuple, type(None))) else None
    return clean, [np.asarray(p) for p in params]


def export_actor_csv(model, out_dir):
    """NN:203-224.  Only the actor is exported, as the reference does."""
    os.makedirs(out_dir, exist_ok=True)
    params = model.get_parameter_list()
    n_layers = len(model.policy.n_lstm)
    for i in range(n_layers):
        np.savetxt(os.path.join(out_dir, "lstm_wx%d.csv" % i), params[3 * i + 0], fmt="%.6f", delimiter=",")
        np.savetxt(os.path.join(out_dir, "lstm_wh%d.csv" % i), params[3 * i + 1], fmt="%.6f", delimiter=",")
        np.savetxt(os.path.join(out_dir, "lstm_b%d.csv" % i), params[3 * i + 2], fmt="%.6f", delimiter=",")
    base = 6 * n_layers
    np.savetxt(os.path.join(out_dir, "pi_w.csv"), params[base + 2], fmt="%.6f", delimiter=",")
    np.savetxt(os.path.join(out_dir, "pi_b.csv"), params[base + 3], fmt="%.6f", delimiter=",")
    return out_dir


class NumpyLstmActor(object):
    """Stateful numpy float64 forward of the LSTM actor (gate order i,f,o,g) for one observation [ob_dim] or a batch [..., ob_dim]: the state
    takes its leading shape from the first observation after a reset().  clip: the output is clipped to [-1, 1] (NN:133-134); the rollout clips
    the sampled action itself (ppo2.py:533) and can switch it off."""

    def __init__(self, wx, wh, b, pi_w, pi_b, clip=True):
        f64 = lambda w: np.asarray(w, np.float64)
        self.wx, self.wh, self.b = [f64(w) for w in wx], [f64(w) for w in wh], [f64(w) for w in b]
        self.pi_w, self.pi_b, self.clip = f64(pi_w), f64(pi_b), clip
        self.reset()

    @classmethod
    def from_csv_dir(cls, d, n_layers=2):
        ld = lambda n: np.loadtxt(os.path.join(d, n), delimiter=",")
        return cls([ld("lstm_wx%d.csv" % i) for i in range(n_layers)], [ld("lstm_wh%d.csv" % i) for i in range(n_layers)],
                   [ld("lstm_b%d.csv" % i) for i in range(n_layers)], ld("pi_w.csv"), ld("pi_b.csv"))

    @classmethod
    def from_parameter_list(cls, params, n_layers=2):
        base = 6 * n_layers
        return cls([params[3 * i] for i in range(n_layers)], [params[3 * i + 1] for i in range(n_layers)],
                   [params[3 * i + 2] for i in range(n_layers)], params[base + 2], params[base + 3])

    @classmethod
    def from_npz(cls, path, clip=True):
        """the actor export of tools/export_actor_fixture.py (tests/golden/actor_*.npz): wx<i>, wh<i>, b<i>, pi_w, pi_b"""
        z = np.load(path)
        layers = range(sum(k.startswith("wx") for k in z.files))
        return cls([z["wx%d" % i] for i in layers], [z["wh%d" % i] for i in layers], [z["b%d" % i] for i in layers], z["pi_w"], z["pi_b"], clip)

    def reset(self):
        self.c = self.h = None

    def act(self, ob, done=None):
        """one step on ob [..., ob_dim]; rows where `done` [...] is set start from a zero state.  -> float64 action [..., act_dim]"""
        x = np.asarray(ob, np.float64)
        if self.c is None:
            self.c = [np.zeros(x.shape[:-1] + (w.shape[0],)) for w in self.wh]
            self.h = [np.zeros(x.shape[:-1] + (w.shape[0],)) for w in self.wh]
        keep = 1.0 if done is None else (~np.asarray(done, bool)).astype(np.float64)[..., None]
        sig = lambda v: 1.0 / (1.0 + np.exp(-v))
        # one vector-matrix product per row: a row's action does not depend on the batch it sits in (a matrix-matrix product sums in another
        # order: rows of a batch of >= 2 differ from the single-vector result by ~1e-14 in this numpy), so a batch IS its rows, bit for bit
        mul = lambda v, w: (v[..., None, :] @ w)[..., 0, :]
        for i in range(len(self.wx)):
            n = self.wh[i].shape[0]
            z = mul(x, self.wx[i]) + mul(self.h[i] * keep, self.wh[i]) + self.b[i]
            ig, fg, og, g = sig(z[..., :n]), sig(z[..., n:2 * n]), sig(z[..., 2 * n:3 * n]), np.tanh(z[..., 3 * n:])
            self.c[i] = fg * (self.c[i] * keep) + ig * g
            self.h[i] = og * np.tanh(self.c[i])
            x = self.h[i]
        a = mul(x, self.pi_w) + self.pi_b
        return np.clip(a, -1.0, 1.0) if self.clip else a

    def predict(self, obs):
        """CustomerLstmNN.predict (NN:112-135): one observation vector -> one action"""
        return self.act(obs)


def mlp_checkpoint_layers(params):
    """does a checkpoint's tensor list have MlpPolicy's shape?  -> (ob_dim, act_dim, layers) or None.  Decided from the arrays' shapes alone:
    an MlpPolicy of the sizes the first arrays suggest is built and the list is held against its sb_parameters(), tensor by tensor."""
    from .policies import MlpPolicy
    shapes = [tuple(np.shape(p)) for p in params]
    if len(shapes) < 12 or len(shapes) % 4 != 3 or len(shapes[0]) != 2 or len(shapes[1]) != 1:
        return None
    n_layers = (len(shapes) - 7) // 4
    layers = tuple(shapes[4 * i][1] for i in range(n_layers) if len(shapes[4 * i]) == 2)
    if len(layers) != n_layers or len(shapes[4 * n_layers + 2]) != 2:
        return None
    ob_dim, act_dim = shapes[0][0], shapes[4 * n_layers + 2][1]
    want = [tuple(p.shape) for p in MlpPolicy(ob_dim=ob_dim, act_dim=act_dim, layers=layers).sb_parameters()]
    squeeze = lambda sh: tuple(d for d in sh if d != 1)
    if len(want) != len(shapes) or any(squeeze(a) != squeeze(b) for a, b in zip(want, shapes)):
        return None
    return ob_dim, act_dim, layers


class NumpyMlpActor(object):
    """numpy float64 forward of MlpPolicy's actor (two tanh layers and the action head) for one observation [ob_dim] or a batch [..., ob_dim]:
    the float64 twin of the device loop's policy step, with NumpyLstmActor's interface -- act(ob, done=None), reset(), predict, clip -- so that
    evaluate.reference_rollout takes either.  The policy has no recurrent state: reset() has nothing to clear and `done` changes nothing."""

    def __init__(self, w, b, pi_w, pi_b, clip=True):
        f64 = lambda a: np.asarray(a, np.float64)
        self.w, self.b = [f64(a) for a in w], [f64(a).reshape(-1) for a in b]
        self.pi_w, self.pi_b, self.clip = f64(pi_w), f64(pi_b).reshape(-1), clip

    @classmethod
    def from_parameter_list(cls, params, n_layers=2, clip=True):
        """MlpPolicy.sb_parameters() order: pi_fc<i> w, b | vf_fc<i> w, b per layer; then vf w, b | pi w, b | logstd | q w, b"""
        base = 4 * n_layers
        return cls([params[4 * i] for i in range(n_layers)], [params[4 * i + 1] for i in range(n_layers)], params[base + 2], params[base + 3], clip)

    @classmethod
    def from_npz(cls, path, clip=True):
        """the actor export of tools/export_actor_fixture.py for an MlpPolicy: pi_w<i>, pi_b<i> (i = 1, 2), pi_w, pi_b"""
        z = np.load(path)
        layers = range(1, 1 + sum(k.startswith("pi_w") and k != "pi_w" for k in z.files))
        return cls([z["pi_w%d" % i] for i in layers], [z["pi_b%d" % i] for i in layers], z["pi_w"], z["pi_b"], clip)

    def reset(self):
        pass

    def act(self, ob, done=None):
        """one step on ob [..., ob_dim]; `done` is accepted for NumpyLstmActor's interface and not read.  -> float64 action [..., act_dim]"""
        x = np.asarray(ob, np.float64)
        # one vector-matrix product per row, so that a batch IS its rows, bit for bit (see NumpyLstmActor.act)
        mul = lambda v, w: (v[..., None, :] @ w)[..., 0, :]
        for w, b in zip(self.w, self.b):
            x = np.tanh(mul(x, w) + b)
        a = mul(x, self.pi_w) + self.pi_b
        return np.clip(a, -1.0, 1.0) if self.clip else a

    def predict(self, obs):
        return self.act(obs)


def numpy_actor(params_or_path, clip=True):
    """the numpy actor a checkpoint's kind asks for: NumpyMlpActor where the tensor list (or the .npz export) is MlpPolicy's, else NumpyLstmActor"""
    if isinstance(params_or_path, str):
        mlp = "pi_w1" in np.load(params_or_path).files
        return (NumpyMlpActor if mlp else NumpyLstmActor).from_npz(params_or_path, clip)
    layers = mlp_checkpoint_layers(params_or_path)
    if layers is not None:
        return NumpyMlpActor.from_parameter_list(params_or_path, len(layers[2]), clip)
    a = NumpyLstmActor.from_parameter_list(params_or_path)
    a.clip = clip
    return a
