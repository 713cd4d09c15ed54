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
// With a scenario (irrl_lstm_eval_scenario: the <true> instantiations of kernels 1 and 5) kernel 1 takes the command target from the step's row of
// the command table and runs the heading hold in lane (e, 2), which owns I_e and reads the base quaternion from the pool's gc; kernel 5 zeroes I_e
// on done and adds the frame into the step's statistics bucket.
// With a kick table (irrl_lstm_eval_perturbed) a step whose row fires gets ONE extra launch, irrl_eval_perturb_kernel, between kernels 3 and 4; a
// step without a kick issues the five launches above.
// A filter coefficient of exactly 1.0f switches that filter OFF (the value passes through bit for bit).  The ring and the two filter histories
// survive an in-episode `done`, as they do in the reference script.
// The per-element arithmetic lives in eval_elements.hpp, ONE text shared with the persistent single-launch form of the same loop
// (irrl_eval_persistent_kernel, env_eval_kernels.hpp: a wave keeps its four robots for all steps; irrl_lstm_eval_rollout_persistent) and with a
// host program: the two device forms leave bit-identical buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/irrl_env.h"
#include "eval_elements.hpp"   // struct EvalArgs and the per-element functions

// steps 1-6 of a control step: a lane per (env, element), so every access to the [D][N][35] ring and to the [N, 35] arrays is coalesced; a lane
// only ever touches its own column of the ring.  SCN: the call has a scenario (irrl_lstm_eval_scenario); the instantiation without one is the loop
// as it was, instruction for instruction
template <bool SCN>
__global__ void __launch_bounds__(256) irrl_eval_condition_kernel(const EvalArgs a) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= a.N * 35) return;
  const int e = i / 35, j = i - e * 35;
  const size_t plane = (size_t)a.N * 35;
  // the scenario's command schedule: lane (e, j < 3) reads its word of this step's table row in place of cmd_target
  const float *target = a.cmd_target + e * 3 + j;
  if (SCN && a.cmd_table && j < 3) target = a.cmd_table + ((size_t)irrl_eval_cmd_row(a, irrl_eval_tau(a, a.t)) * (size_t)a.N + (size_t)e) * 3 + j;
  float o = irrl_eval_condition_element(a, a.slot, j, a.obs[i], a.ring + i, plane, a.delay[e], a.vel_his + i, a.cmd + e * 3 + j, target);
  // the heading hold: lane (e, 2) owns I_e; the base quaternion is the pool's (the state after the previous step or the reset)
  if (SCN && a.heading_kp && j == 2) {
    const float kp = a.heading_kp[e], ki = a.heading_ki[e];
    if (irrl_eval_heading_on(kp, ki)) {
      const float *q = a.gc + e * 19 + 3;
      o = irrl_eval_heading_element(a, a.heading_ref[e], kp, ki, q[0], q[1], q[2], q[3], a.heading_int + e);
    }
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
  const float y = irrl_eval_action_element(a.a_act, x, a.act_his + i);
  a.applied[i] = y;
  if (a.rec_act_clipped) a.rec_act_clipped[r] = x;
  if (a.rec_act_applied) a.rec_act_applied[r] = y;
}

// steps 12-13, after the env step: the recorders (a lane per element of the widest one), and in the lanes e < N the command reset and the
// statistics -- one lane owns env e's column of `stats`, no atomics
template <bool SCN>
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
  const float *gc = a.gc + e * 19, *gv = a.gv + e * 18;
  if (SCN && a.heading_int) irrl_eval_heading_epilogue(dn != 0, a.heading_int + e);
  // the frame goes to this step's bucket of the statistics (no scenario: bucket 0, the whole buffer)
  const size_t bucket = SCN ? (size_t)irrl_eval_stat_bucket(a, irrl_eval_tau(a, a.t)) * (size_t)IRRL_EVAL_STAT_COUNT * (size_t)N : (size_t)0;
  irrl_eval_env_epilogue(dn != 0, a.cmd + e * 3, a.stats ? a.stats + bucket + e : nullptr, (size_t)N, gc[2], gc[3], gc[4], gc[5], gc[6], gv[0], gv[1], gv[2], gv[3], gv[4], gv[5]);
  // the gait measurements (irrl_lstm_eval_measured): the same lane owns env e's column of `gait`, its prev_contact bytes and its recorder row
  if (a.gait || a.rec_gait || a.prev_contact) {
    const float *tq = a.torque + (size_t)e * 12, *lamw = a.lam_w + (size_t)e * 12;
    const int *ic = a.in_contact + (size_t)e * 4;
    if (a.rec_gait) irrl_eval_gait_record(a.rec_gait + (row * (size_t)N + (size_t)e) * IRRL_EVAL_GAIT_REC_DIM, tq, gv + 6, ic, lamw, a.inv_control_dt);
    const size_t gbucket = SCN ? (size_t)irrl_eval_stat_bucket(a, irrl_eval_tau(a, a.t)) * (size_t)IRRL_EVAL_GAIT_COUNT * (size_t)N : (size_t)0;
    irrl_eval_gait_epilogue(dn != 0, a.gait ? a.gait + gbucket + e : nullptr, (size_t)N, a.prev_contact ? a.prev_contact + (size_t)e * 4 : nullptr, tq, gv + 6, ic,
                            lamw, a.inv_control_dt);
  }
}

// a kick row per env on the pool's base state (irrl_env_perturb_base; the extra launch of irrl_lstm_eval_perturbed at a step whose row fires,
// between the action filter and the env step): a lane per env, which owns that env's gc[2:7] and gv[0:6].  Any pool kind and lane layout:
// gc / gv are [N, 19] / [N, 18] in every one.  An env whose row is off is not written.
__global__ void __launch_bounds__(256) irrl_eval_perturb_kernel(int N, const float *rows, float *gc_, float *gv_) {
  const int e = (int)(blockIdx.x * 256u + threadIdx.x);
  if (e >= N) return;
  const float *k = rows + (size_t)e * IRRL_EVAL_KICK_DIM;
  if (!irrl_eval_kick_on(k)) return;
  float *gc = gc_ + (size_t)e * 19, *gv = gv_ + (size_t)e * 18;
  float pz = gc[2], w = gc[3], x = gc[4], y = gc[5], z = gc[6], v0 = gv[0], v1 = gv[1], v2 = gv[2], o0 = gv[3], o1 = gv[4], o2 = gv[5];
  irrl_eval_kick_apply(k, pz, w, x, y, z, v0, v1, v2, o0, o1, o2);
  gc[2] = pz; gc[3] = w; gc[4] = x; gc[5] = y; gc[6] = z;
  gv[0] = v0; gv[1] = v1; gv[2] = v2; gv[3] = o0; gv[4] = o1; gv[5] = o2;
}

// the trace recorders' row of one step (irrl_eval_trace, include/irrl_env.h; the extra launch of irrl_lstm_eval_traced / irrl_mlp_eval_traced between
// the policy step and the action filter): a lane per (env, column < hid4) copies the actor's half of the recurrent state, lstm_state[e, 0 : hid4]
// of [N, 2 hid4], and the lanes e < N the critic's value -- reads and writes both run along the lanes.  Either row pointer may be NULL.
__global__ void __launch_bounds__(256) irrl_eval_trace_kernel(int N, int hid4, const float *lstm_state, const float *value, float *rec_lstm_row,
                                                              float *rec_value_row) {
  const size_t i = (size_t)blockIdx.x * 256u + (size_t)threadIdx.x;
  if (rec_lstm_row && i < (size_t)N * (size_t)hid4) {
    const size_t e = i / (size_t)hid4, j = i - e * (size_t)hid4;
    rec_lstm_row[i] = lstm_state[e * 2 * (size_t)hid4 + j];
  }
  if (rec_value_row && i < (size_t)N) rec_value_row[i] = value[i];
}

static inline dim3 eval_grid(int n_elems) { return dim3((unsigned)((n_elems + 255) / 256)); }
