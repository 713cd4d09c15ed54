"""Extract the actor tensors of a PPO2 checkpoint of this build into an .npz fixture: the eight of a CustomLSTMPolicy (same layout as
tests/golden/actor_bp5_155.npz), or the six of an MlpPolicy (pi_w1, pi_b1, pi_w2, pi_b2, pi_w, pi_b) -- by the checkpoint's kind.
usage: python tools/export_actor_fixture.py ckpt.pkl out.npz"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from high_speed_quadrupedal_locomotion_by_irrl_amd.checkpoint import mlp_checkpoint_layers, read_checkpoint

_, params = read_checkpoint(sys.argv[1])
params = [np.asarray(p, np.float32) for p in params]
if mlp_checkpoint_layers(params) is not None:      # MlpPolicy.sb_parameters(): pi_fc<i> w, b | vf_fc<i> w, b per layer; vf w, b | pi w, b | ...
    out = {"pi_w1": params[0], "pi_b1": params[1], "pi_w2": params[4], "pi_b2": params[5], "pi_w": params[10], "pi_b": params[11]}
else:
    out = {n: params[i] for i, n in enumerate(["wx0", "wh0", "b0", "wx1", "wh1", "b1"])}
    out["pi_w"], out["pi_b"] = params[14], params[15]
np.savez_compressed(sys.argv[2], **out)
print("wrote", sys.argv[2], {k: v.shape for k, v in out.items()})
