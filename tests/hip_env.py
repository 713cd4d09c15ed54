"""Test adapter: the product path (HIP kernels behind the C-ABI, via the reference-style FlexibleGymEnv
shim) wrapped to the tiny interface parity_lib.py drives.  Imports nothing from oracle/."""
import numpy as np
import yaml

import high_speed_quadrupedal_locomotion_by_irrl_amd as pkg
from high_speed_quadrupedal_locomotion_by_irrl_amd.flexible_robot import FlexibleGymEnv


class HipVecEnv(object):
    def __init__(self, env_cfg):
        env_cfg = dict(env_cfg)
        ref = env_cfg.pop("_ref_table", None)     # reference-trajectory table of a ManualTraj: False config (test plumbing)
        # one line per key: the library's config reader takes "key: value" lines, and PyYAML would otherwise fold a long value
        # (a RefTraj path with a space, under a long temporary directory) onto a second line
        text = yaml.safe_dump(env_cfg, default_flow_style=False, width=float("inf"))
        self.impl = FlexibleGymEnv(pkg.__BLACKPANTHER_V55_RESOURCE_DIRECTORY__, text)
        if ref is not None:
            self.impl.set_ref(ref)
        self.impl.init()
        self.n = self.impl.getNumOfEnvs()
        self._ob = np.zeros((self.n, 35), np.float32)
        self._rew = np.zeros(self.n, np.float32)
        self._done = np.zeros(self.n, np.bool_)
        self._extra = np.zeros((self.n, 6), np.float32)

    def observe(self):
        self.impl.observe(self._ob)
        return self._ob.copy()

    def reset(self):
        self.impl.reset(self._ob)
        return self._ob.copy()

    def step(self, action):
        self.impl.step(np.ascontiguousarray(action, np.float32), self._ob, self._rew, self._done, self._extra)
        return self._ob.copy(), self._rew.copy(), self._done.copy(), self._extra.copy()

    def probe(self):
        minv = np.zeros((self.n, 324), np.float32)
        nl = np.zeros((self.n, 18), np.float32)
        self.impl.GetInverseMassMatrix(minv)
        self.impl.GetNonlinear(nl)
        return minv, nl

    def sphere_info(self):
        out = np.zeros((self.n, 4), np.float32)
        self.impl.GetSphereInfo(out)
        return out

    def joint_effort(self):
        out = np.zeros((self.n, 12), np.float32)
        self.impl.GetJointEffort(out)
        return out

    def get_state(self):
        return self.impl.get_state()

    def set_contact_coeff(self, coeff):
        self.impl.SetContactCoefficient(np.ascontiguousarray(coeff, np.float32))

    def set_state(self, st):
        self.impl.set_state(st)
