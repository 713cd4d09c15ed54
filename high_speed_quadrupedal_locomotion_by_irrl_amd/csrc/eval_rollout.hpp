// eval_rollout.hpp -- the device-resident evaluation loop of a trained policy (irrl_lstm_eval_rollout, include/irrl_env.h): what the reference's
// evaluation script does on the host around every control step (run_bp_v5.py:353-470: command low-pass, observation delay line = DelayTool.py:5-21,
// rate / action low-passes, per-step records), as three small kernels that sit between the existing policy-step and env-step launches.
//
// One control step t = five launches on the caller's stream, no graph, no host round trip:
//   1. irrl_eval_condition_kernel   cmd filter, ring[t % D] = obs, o = ring[(t - delay_e) mod D], rate low-pass, vel_his = o, o[0:3] = scaled command
//   2. the policy step              (lstm_kernels.hip lstm_policy_step_kernel, deterministic; resets the LSTM state of an env whose `done` is set)
//   3. irrl_eval_action_kernel      action low-pass, act_his, the action buffer the env step reads
//   4. the env step                 (launch_step of irrl_env_abi.hip: whatever kernel variant and lane layout the pool runs)
//   5. irrl_eval_record_kernel      recorders, cmd = 0 on done, per-env f64 statistics
// A filter coefficient of exactly 1.0f switches that filter OFF (the value passes through bit for bit).  The ring and the two filter histories
// survive an in-episode `done`, as they do in the reference script.
// OUT OF SCOPE here: a persistent single-launch form of the whole evaluation (the env kernels are not touched by this file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/irrl_env.h"

struct EvalArgs {
  int N, D;
  int slot;          // t % D: the ring plane this step writes
  long long row;     // row of the recorders this step fills
  // evaluator state
  float *ring;       // [D, N, 35]
  float *cmd;        // [N, 3] low-passed command
  float *vel_his;    // [N, 35] previous conditioned observation
  float *act_his;    // [N, 12] previous applied action
  const float *obs;  // [N, 35] raw observation (the env step's output)
  const uint8_t *done;   // [N]
  // per-env parameters
  const int *delay;          // [N], 0 .. D-1 (clamped here: a bad value must not become an out-of-bounds plane)
  const float *cmd_target;   // [N, 3]
  float a_cmd, a_vel, a_act;
  float mean0, mean1, mean2, std0, std1, std2;   // scaling of obs[0:3]
  // work arrays
  float *obs_cond;        // [N, 35] what the policy step reads
  const float *act_in;    // [N, 12] the actor's output (clipped mean, or the mean)
  float *applied;         // [N, 12] what the env step reads
  const float *reward;    // [N]
  // the pool (after the env step)
  const float *gc, *gv, *torque;
  // recorders, each may be NULL
  float *rec_obs_cond, *rec_act_clipped, *rec_act_applied, *rec_body, *rec_torque, *rec_obs_raw, *rec_reward;
  uint8_t *rec_done;
  double *stats;     // [IRRL_EVAL_STAT_COUNT, N] or NULL
};

// steps 1-6 of a control step: a lane per (env, element), so every access to the [D][N][35] ring and to the [N, 35] arrays is coalesced; a lane
// only ever touches its own column of the ring
__global__ void __launch_bounds__(256) irrl_eval_condition_kernel(const EvalArgs a) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= a.N * 35) return;
  const int e = i / 35, j = i - e * 35;
  const size_t plane = (size_t)a.N * 35;
  const float raw = a.obs[i];
  a.ring[(size_t)a.slot * plane + (size_t)i] = raw;
  int d = a.delay[e];
  d = d < 0 ? 0 : d > a.D - 1 ? a.D - 1 : d;
  int slot_r = a.slot - d;
  if (slot_r < 0) slot_r += a.D;
  float o = d == 0 ? raw : a.ring[(size_t)slot_r * plane + (size_t)i];
  const bool rate = (j >= 17 && j < 29) || j >= 32;     // joint rates, body angular velocity
  if (rate && a.a_vel != 1.0f) o = (1.0f - a.a_vel) * a.vel_his[i] + a.a_vel * o;
  a.vel_his[i] = o;                                     // the whole vector, before the command overwrite
  if (j < 3) {
    const float target = a.cmd_target[e * 3 + j];
    const float c = a.a_cmd != 1.0f ? (1.0f - a.a_cmd) * a.cmd[e * 3 + j] + a.a_cmd * target : target;
    a.cmd[e * 3 + j] = c;
    o = (c - (j == 0 ? a.mean0 : j == 1 ? a.mean1 : a.mean2)) / (j == 0 ? a.std0 : j == 1 ? a.std1 : a.std2);
  }
  a.obs_cond[i] = o;
  if (a.rec_obs_cond) a.rec_obs_cond[(size_t)a.row * plane + (size_t)i] = o;
}

// steps 9-10: the action low-pass between the policy step and the env step
__global__ void __launch_bounds__(256) irrl_eval_action_kernel(const EvalArgs a) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= a.N * 12) return;
  const size_t r = (size_t)a.row * (size_t)a.N * 12 + (size_t)i;
  const float x = a.act_in[i];
  const float y = a.a_act != 1.0f ? (1.0f - a.a_act) * a.act_his[i] + a.a_act * x : x;
  a.act_his[i] = y;
  a.applied[i] = y;
  if (a.rec_act_clipped) a.rec_act_clipped[r] = x;
  if (a.rec_act_applied) a.rec_act_applied[r] = y;
}

// steps 12-13, after the env step: the recorders (a lane per element of the widest one), and in the lanes e < N the command reset and the
// statistics -- one lane owns env e's column of `stats`, no atomics
__global__ void __launch_bounds__(256) irrl_eval_record_kernel(const EvalArgs a) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  const int N = a.N;
  const size_t row = (size_t)a.row;
  if (i >= N * 35) return;
  if (a.rec_obs_raw) a.rec_obs_raw[row * (size_t)N * 35 + (size_t)i] = a.obs[i];
  if (a.rec_body && i < N * 13) {                        // base x y z, quaternion wxyz | world linear and angular velocity
    const int e = i / 13, j = i - e * 13;
    a.rec_body[row * (size_t)N * 13 + (size_t)i] = j < 7 ? a.gc[e * 19 + j] : a.gv[e * 18 + j - 7];
  }
  if (a.rec_torque && i < N * 12) a.rec_torque[row * (size_t)N * 12 + (size_t)i] = a.torque[i];
  if (i >= N) return;
  const int e = i;
  const uint8_t dn = a.done[e];
  if (a.rec_reward) a.rec_reward[row * (size_t)N + (size_t)e] = a.reward[e];
  if (a.rec_done) a.rec_done[row * (size_t)N + (size_t)e] = dn;
  if (dn) { a.cmd[e * 3 + 0] = 0.0f; a.cmd[e * 3 + 1] = 0.0f; a.cmd[e * 3 + 2] = 0.0f; }   // the env restarted from rest
  if (!a.stats) return;
  // world -> body frame, roll and pitch in f64 from the f32 samples
  const double pz = a.gc[e * 19 + 2];
  const double w = a.gc[e * 19 + 3], x = a.gc[e * 19 + 4], y = a.gc[e * 19 + 5], z = a.gc[e * 19 + 6];
  const double v0 = a.gv[e * 18 + 0], v1 = a.gv[e * 18 + 1], v2 = a.gv[e * 18 + 2];
  const double o0 = a.gv[e * 18 + 3], o1 = a.gv[e * 18 + 4], o2 = a.gv[e * 18 + 5];
  const double r00 = 1 - 2 * (y * y + z * z), r01 = 2 * (x * y - w * z);
  const double r10 = 2 * (x * y + w * z), r11 = 1 - 2 * (x * x + z * z);
  const double r20 = 2 * (x * z - w * y), r21 = 2 * (w * x + y * z);
  const double vx = r00 * v0 + r10 * v1 + r20 * v2, vy = r01 * v0 + r11 * v1 + r21 * v2;
  const double wx = r00 * o0 + r10 * o1 + r20 * o2, wy = r01 * o0 + r11 * o1 + r21 * o2;
  const double roll = atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y));
  double sp = 2 * (w * y - x * z);
  sp = sp > 1.0 ? 1.0 : sp < -1.0 ? -1.0 : sp;
  const double pitch = asin(sp);
  double *s = a.stats + e;
  const size_t n = (size_t)N;
  s[IRRL_EVAL_STAT_N * n] += 1.0;
  s[IRRL_EVAL_STAT_VX * n] += vx; s[IRRL_EVAL_STAT_VX2 * n] += vx * vx;
  s[IRRL_EVAL_STAT_Z * n] += pz; s[IRRL_EVAL_STAT_Z2 * n] += pz * pz;
  s[IRRL_EVAL_STAT_ROLL * n] += roll; s[IRRL_EVAL_STAT_ROLL2 * n] += roll * roll;
  s[IRRL_EVAL_STAT_PITCH * n] += pitch; s[IRRL_EVAL_STAT_PITCH2 * n] += pitch * pitch;
  s[IRRL_EVAL_STAT_WX * n] += wx; s[IRRL_EVAL_STAT_WX2 * n] += wx * wx;
  s[IRRL_EVAL_STAT_WY * n] += wy; s[IRRL_EVAL_STAT_WY2 * n] += wy * wy;
  s[IRRL_EVAL_STAT_VZ * n] += v2; s[IRRL_EVAL_STAT_VZ2 * n] += v2 * v2;
  s[IRRL_EVAL_STAT_VY * n] += vy;
  s[IRRL_EVAL_STAT_WZ * n] += o2;
  s[IRRL_EVAL_STAT_FALLS * n] += dn ? 1.0 : 0.0;
}

static inline dim3 eval_grid(int n_elems) { return dim3((unsigned)((n_elems + 255) / 256)); }
