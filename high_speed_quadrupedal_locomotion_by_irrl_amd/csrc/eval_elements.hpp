// eval_elements.hpp -- the per-element arithmetic of the evaluation loop (irrl_lstm_eval_rollout[_persistent], include/irrl_env.h) in ONE text:
// the three small kernels of eval_rollout.hpp and the persistent kernel of env_eval_kernels.hpp call these functions, and so does a host
// program (tests/eval_elements_main.cpp) -- this header includes no HIP header and compiles with any C++ compiler.
// The library is built with -ffp-contract=on: a multiply-add fuses where the source writes a * b + c in ONE expression and nowhere else, so the
// shape of the expressions below is part of the contract between the two device forms (bit-identical buffers).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/irrl_env.h"

#ifdef __HIPCC__
#define IRRL_EVAL_FN __host__ __device__
#else
#define IRRL_EVAL_FN
#endif

struct EvalArgs {
  int N, D;
  int slot;          // t % D: the ring plane this step (the persistent kernel: its first step) writes
  int steps;         // the persistent kernel's step count (the per-step kernels do not read it)
  int clip;          // the persistent kernel: apply the [-1, 1] clipped action (the per-step kernels get act_in chosen by the host)
  long long row;     // row of the recorders this step (the persistent kernel: its first step) fills
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
  double *stats;     // [IRRL_EVAL_STAT_COUNT, N] or NULL; with a scenario [stat_buckets, IRRL_EVAL_STAT_COUNT, N]
  // the scenario (irrl_eval_scenario, include/irrl_env.h); all zero / NULL = none: a value-initialised EvalArgs is the loop without one
  long long t;       // global control step of this step (the persistent kernel: of its first step)
  long long t0;      // the scenario's origin: tau = max(t - t0, 0)
  int cmd_rows, cmd_every;          // the command schedule; read only where cmd_table is set
  const float *cmd_table;           // [cmd_rows, N, 3] or NULL: cmd_target is the target
  int stat_buckets, stat_every;     // stat_buckets < 1: one bucket
  const float *heading_ref, *heading_kp, *heading_ki;   // [N] each, or all NULL: heading hold off
  float *heading_int;               // [N] the integrator I
  float heading_windup, heading_dt;
  // the kick table (irrl_eval_kicks, include/irrl_env.h); kick_table NULL = none.  Its schedule counts from t0 above (0 without a scenario)
  int kick_rows, kick_every;        // read only where kick_table is set
  long long kick_first;
  const float *kick_table;          // [kick_rows, N, IRRL_EVAL_KICK_DIM] or NULL
  // the gait measurements (irrl_eval_gait, include/irrl_env.h); all three NULL = none.  The buckets are the statistics' (stat_buckets, stat_every)
  double *gait;                     // [stat_buckets, IRRL_EVAL_GAIT_COUNT, N] or NULL
  uint8_t *prev_contact;            // [N, 4] the contact flags of the previous step (NULL with the recorder alone)
  float *rec_gait;                  // [steps, N, IRRL_EVAL_GAIT_REC_DIM] or NULL
  const int *in_contact;            // the pool (after the env step): [N, 4] contact flags, [N, 4, 3] world-frame impulses of the last substep
  const float *lam_w;
  float inv_control_dt;
};

// steps 1-6 of a control step for ONE element (env e, component j) of the observation: ring[slot] = raw, the delayed read, the rate low-pass,
// vel_his, and for j < 3 the command low-pass and its scaling.  ring_i: the element's column of the ring (ring + e * 35 + j; planes are
// `plane` = N * 35 floats apart); vel_his_i / cmd_ej / target_ej: the element's own words (cmd_ej and target_ej are read for j < 3 only).
// A delay outside 0 .. D-1 is clamped.  -> what the actor sees.
static inline IRRL_EVAL_FN float irrl_eval_condition_element(const EvalArgs &a, int slot, int j, float raw, float *ring_i, size_t plane, int delay_e,
                                                             float *vel_his_i, float *cmd_ej, const float *target_ej) {
  ring_i[(size_t)slot * plane] = raw;
  int d = delay_e;
  d = d < 0 ? 0 : d > a.D - 1 ? a.D - 1 : d;
  int slot_r = slot - d;
  if (slot_r < 0) slot_r += a.D;
  float o = d == 0 ? raw : ring_i[(size_t)slot_r * plane];
  const bool rate = (j >= 17 && j < 29) || j >= 32;     // joint rates, body angular velocity
  if (rate && a.a_vel != 1.0f) o = (1.0f - a.a_vel) * *vel_his_i + a.a_vel * o;
  *vel_his_i = o;                                       // the whole vector, before the command overwrite
  if (j < 3) {
    const float target = *target_ej;
    const float c = a.a_cmd != 1.0f ? (1.0f - a.a_cmd) * *cmd_ej + a.a_cmd * target : target;
    *cmd_ej = c;
    o = (c - (j == 0 ? a.mean0 : j == 1 ? a.mean1 : a.mean2)) / (j == 0 ? a.std0 : j == 1 ? a.std1 : a.std2);
  }
  return o;
}

// steps 9-10 for ONE action element: the low-pass between the policy step and the env step; act_his_i is updated.  -> the applied action
static inline IRRL_EVAL_FN float irrl_eval_action_element(float a_act, float x, float *act_his_i) {
  const float y = a_act != 1.0f ? (1.0f - a_act) * *act_his_i + a_act * x : x;
  *act_his_i = y;
  return y;
}

// steps 12-13 for ONE env, after the env step: cmd = 0 on done, and (s != NULL) the statistics of the body frame -- world -> body frame, roll and
// pitch in f64 from the f32 samples, added to the env's column s[slot * n].  pz: base height; w x y z: the base quaternion; v0 v1 v2 / o0 o1 o2:
// world linear / angular velocity.
static inline IRRL_EVAL_FN void irrl_eval_env_epilogue(bool dn, float *cmd_e, double *s, size_t n, float pz_, float w_, float x_, float y_, float z_,
                                                       float v0_, float v1_, float v2_, float o0_, float o1_, float o2_) {
  if (dn) { cmd_e[0] = 0.0f; cmd_e[1] = 0.0f; cmd_e[2] = 0.0f; }   // the env restarted from rest
  if (!s) return;
  const double pz = pz_;
  const double w = w_, x = x_, y = y_, z = z_;
  const double v0 = v0_, v1 = v1_, v2 = v2_;
  const double o0 = o0_, o1 = o1_, o2 = o2_;
  const double r00 = 1 - 2 * (y * y + z * z), r01 = 2 * (x * y - w * z);
  const double r10 = 2 * (x * y + w * z), r11 = 1 - 2 * (x * x + z * z);
  const double r20 = 2 * (x * z - w * y), r21 = 2 * (w * x + y * z);
  const double vx = r00 * v0 + r10 * v1 + r20 * v2, vy = r01 * v0 + r11 * v1 + r21 * v2;
  const double wx = r00 * o0 + r10 * o1 + r20 * o2, wy = r01 * o0 + r11 * o1 + r21 * o2;
  const double roll = atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y));
  double sp = 2 * (w * y - x * z);
  sp = sp > 1.0 ? 1.0 : sp < -1.0 ? -1.0 : sp;
  const double pitch = asin(sp);
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

// ---- the scenario: command schedule, heading hold, statistics buckets ----
// tau of control step t: steps since the scenario's origin, 0 in front of it
static inline IRRL_EVAL_FN long long irrl_eval_tau(const EvalArgs &a, long long t) { return t > a.t0 ? t - a.t0 : 0; }
// the row of cmd_table that step tau reads: min(tau / cmd_every, cmd_rows - 1) -- the last row holds once the table runs out
static inline IRRL_EVAL_FN int irrl_eval_cmd_row(const EvalArgs &a, long long tau) {
  const long long r = tau / (long long)a.cmd_every;
  return r < (long long)(a.cmd_rows - 1) ? (int)r : a.cmd_rows - 1;
}
// the bucket of `stats` the frame of step tau is added to: min(tau / stat_every, stat_buckets - 1); no buckets (< 1): 0
static inline IRRL_EVAL_FN int irrl_eval_stat_bucket(const EvalArgs &a, long long tau) {
  if (a.stat_buckets < 1) return 0;
  const long long b = tau / (long long)a.stat_every;
  return b < (long long)(a.stat_buckets - 1) ? (int)b : a.stat_buckets - 1;
}
// is the heading hold on for an env with these gains
static inline IRRL_EVAL_FN bool irrl_eval_heading_on(float kp, float ki) { return kp != 0.0f || ki != 0.0f; }
// Heading hold for ONE env (run_bp_v5.py:308-315, 400-406: a PI loop on the base yaw of utils/Rotation.py:8 whose output replaces the yaw-rate
// command the actor sees).  The reference's utils/PID.py is not in its tree; the rule here is the common positional PID with Kd = 0 and an
// integrator clamp: err = wrap(ref - yaw) into [-pi, pi), I = clamp(I + err dt, -W, W), out = kp err + ki I.  w x y z: the base quaternion as the
// pool holds it at conditioning time (the state after the previous step, or after the reset; not delayed).  *I_e is updated.
// -> the actor's element 2, (out - mean2) / std2.  f32, every statement ONE expression (see the note on -ffp-contract at the top).
static inline IRRL_EVAL_FN float irrl_eval_heading_element(const EvalArgs &a, float ref, float kp, float ki, float w, float x, float y, float z, float *I_e) {
  const float pi = 3.14159265358979323846f, two_pi = 6.28318530717958647692f;
  const float yaw = atan2f(2.0f * (w * z + x * y), 1.0f - 2.0f * (y * y + z * z));
  const float d = ref - yaw;
  float err = d - two_pi * floorf((d + pi) / two_pi);
  err = err >= pi ? err - two_pi : err < -pi ? err + two_pi : err;       // (the rounding of the line above can leave the interval by an ulp)
  const float I = fminf(fmaxf(*I_e + err * a.heading_dt, -a.heading_windup), a.heading_windup);
  *I_e = I;
  const float out = kp * err + ki * I;
  return (out - a.mean2) / a.std2;
}
// after the env step: the env restarted from rest, so does its integrator
static inline IRRL_EVAL_FN void irrl_eval_heading_epilogue(bool dn, float *I_e) {
  if (dn) *I_e = 0.0f;
}

// ---- the kick table: caller-specified base-state displacements at chosen control steps (irrl_eval_kicks, include/irrl_env.h) ----
// the row of kick_table that fires at control step t, or -1: row r fires where t >= t0 + kick_first and t - t0 - kick_first = r kick_every with
// 0 <= r < kick_rows.  Written in t, not in tau: tau is clamped to 0 in front of t0, where a rule in tau would fire at every step.
static inline IRRL_EVAL_FN int irrl_eval_kick_row(const EvalArgs &a, long long t) {
  const long long d = t - a.t0 - a.kick_first;
  if (d < 0) return -1;
  const long long r = d / (long long)a.kick_every;
  if (r * (long long)a.kick_every != d || r >= (long long)a.kick_rows) return -1;
  return (int)r;
}
// does the row displace its env: a row whose four dq words are all zero is "no kick for this env", whatever its other seven words are
static inline IRRL_EVAL_FN bool irrl_eval_kick_on(const float *k) { return k[1] != 0.0f || k[2] != 0.0f || k[3] != 0.0f || k[4] != 0.0f; }
// One kick row k = dz | dq_w dq_x dq_y dq_z | dv_x dv_y dv_z | dw_x dw_y dw_z on ONE env's base state, body-frame: with R(q) the rotation matrix
// of the base quaternion BEFORE the kick,  z += dz,  v_w += R(q) dv,  w_w += R(q) dw,  q = (q (x) dq) / |q (x) dq|.  pz: base height; w x y z: the
// base quaternion; v0 v1 v2 / o0 o1 o2: world linear / angular velocity (gc[2], gc[3:7], gv[0:3], gv[3:6]); nothing else of the env is touched,
// and an env whose row is off (irrl_eval_kick_on) keeps its ten words bit for bit.  No trigonometry: dq comes from the host.
// f32, every statement ONE expression (see the note on -ffp-contract at the top); the norm as 1.0f / sqrtf(n).
static inline IRRL_EVAL_FN void irrl_eval_kick_apply(const float *k, float &pz, float &w, float &x, float &y, float &z, float &v0, float &v1, float &v2,
                                                     float &o0, float &o1, float &o2) {
  if (!irrl_eval_kick_on(k)) return;
  const float dz = k[0], dw = k[1], dx = k[2], dy = k[3], dq = k[4];
  const float r00 = 1.0f - 2.0f * (y * y + z * z);
  const float r01 = 2.0f * (x * y - w * z);
  const float r02 = 2.0f * (x * z + w * y);
  const float r10 = 2.0f * (x * y + w * z);
  const float r11 = 1.0f - 2.0f * (x * x + z * z);
  const float r12 = 2.0f * (y * z - w * x);
  const float r20 = 2.0f * (x * z - w * y);
  const float r21 = 2.0f * (y * z + w * x);
  const float r22 = 1.0f - 2.0f * (x * x + y * y);
  pz = pz + dz;
  v0 = v0 + (r00 * k[5] + r01 * k[6] + r02 * k[7]);
  v1 = v1 + (r10 * k[5] + r11 * k[6] + r12 * k[7]);
  v2 = v2 + (r20 * k[5] + r21 * k[6] + r22 * k[7]);
  o0 = o0 + (r00 * k[8] + r01 * k[9] + r02 * k[10]);
  o1 = o1 + (r10 * k[8] + r11 * k[9] + r12 * k[10]);
  o2 = o2 + (r20 * k[8] + r21 * k[9] + r22 * k[10]);
  const float qw = w * dw - x * dx - y * dy - z * dq;
  const float qx = w * dx + x * dw + y * dq - z * dy;
  const float qy = w * dy - x * dq + y * dw + z * dx;
  const float qz = w * dq + x * dy - y * dx + z * dw;
  const float n = qw * qw + qx * qx + qy * qy + qz * qz;
  const float s = 1.0f / sqrtf(n);
  w = qw * s;
  x = qx * s;
  y = qy * s;
  z = qz * s;
}

// ---- the gait measurements: joint power, torque and ground-force sums, footfall pattern at control-step rate (irrl_eval_gait, include/irrl_env.h) ----
// the four lam_w_z words of the recorder: the f32 product the GRFZ row widens
static inline IRRL_EVAL_FN float irrl_eval_gait_fz(float lamw_z, float inv_control_dt) { return lamw_z * inv_control_dt; }
// For ONE env, after the env step: tq / qd [12] (joint j = 3 leg + k; S.torque, gv[6:18]), in_contact [4], lamw [4][3] as the pool holds them, dn the
// step's `done`.  g: the env's column of this step's bucket of `gait` (rows n words apart) or NULL; prev: the env's four prev_contact bytes or NULL.
// A step that ends in `done` adds nothing and still sets prev := in_contact.  Every f32 word is widened to f64 first -- the products of two widened
// words are exact -- and every sum is added in index order, so the rows N, P, PPOS, PNEG, STANCE, TOUCHDOWN, FLIGHT, GRFZ and the peaks of |tq|, |qd| are
// the same on every machine; every square and every product that is rounded stands in a statement of its own (see the note on -ffp-contract at the top).
static inline IRRL_EVAL_FN void irrl_eval_gait_epilogue(bool dn, double *g, size_t n, uint8_t *prev, const float *tq, const float *qd, const int *in_contact,
                                                        const float *lamw, float inv_control_dt) {
  if (g && !dn) {
    double p = 0.0, ppos = 0.0, pneg = 0.0, tau2 = 0.0, tau2k = 0.0, ptau = 0.0, pqd = 0.0;
    for (int j = 0; j < 12; j++) {
      const double t = (double)tq[j], w = (double)qd[j];
      const double tw = t * w;          // exact: 24 x 24 bits
      p += tw;
      if (tw > 0.0) ppos += tw;
      if (tw < 0.0) pneg += tw;
      const double tt = t * t;          // exact
      if (j % 3 == 2) tau2k += tt; else tau2 += tt;
      const double at = fabs(t), aw = fabs(w);
      if (at > ptau) ptau = at;
      if (aw > pqd) pqd = aw;
    }
    const double pp = p * p;
    g[IRRL_EVAL_GAIT_N * n] += 1.0;
    g[IRRL_EVAL_GAIT_P * n] += p;
    g[IRRL_EVAL_GAIT_P2 * n] += pp;
    g[IRRL_EVAL_GAIT_PPOS * n] += ppos;
    g[IRRL_EVAL_GAIT_PNEG * n] += pneg;
    g[IRRL_EVAL_GAIT_TAU2 * n] += tau2;
    g[IRRL_EVAL_GAIT_TAU2_KNEE * n] += tau2k;
    if (ptau > g[IRRL_EVAL_GAIT_PEAK_TAU * n]) g[IRRL_EVAL_GAIT_PEAK_TAU * n] = ptau;
    if (pqd > g[IRRL_EVAL_GAIT_PEAK_QD * n]) g[IRRL_EVAL_GAIT_PEAK_QD * n] = pqd;
    double grfz = 0.0, pgrf = 0.0;
    bool any = false;
    for (int l = 0; l < 4; l++) {
      if (in_contact[l] == 0) continue;
      any = true;
      g[(IRRL_EVAL_GAIT_STANCE0 + l) * n] += 1.0;
      if (prev && prev[l] == 0) g[(IRRL_EVAL_GAIT_TOUCHDOWN0 + l) * n] += 1.0;
      const float fz = irrl_eval_gait_fz(lamw[l * 3 + 2], inv_control_dt);
      grfz += (double)fz;
      const double lx = (double)lamw[l * 3], ly = (double)lamw[l * 3 + 1], lz = (double)lamw[l * 3 + 2];
      const double xx = lx * lx;
      const double yy = ly * ly;
      const double zz = lz * lz;
      const double xy = xx + yy;
      const double n2 = xy + zz;
      const double nr = sqrt(n2);
      const double f = nr * (double)inv_control_dt;
      if (f > pgrf) pgrf = f;
    }
    if (!any) g[IRRL_EVAL_GAIT_FLIGHT * n] += 1.0;
    g[IRRL_EVAL_GAIT_GRFZ * n] += grfz;
    if (pgrf > g[IRRL_EVAL_GAIT_PEAK_GRF * n]) g[IRRL_EVAL_GAIT_PEAK_GRF * n] = pgrf;
  }
  if (prev)
    for (int l = 0; l < 4; l++) prev[l] = in_contact[l] != 0 ? 1 : 0;
}
// the recorder's row of ONE env out of the same words: tq 12 | qd 12 | in_contact 4 | lam_w_z / control_dt 4
static inline IRRL_EVAL_FN void irrl_eval_gait_record(float *r, const float *tq, const float *qd, const int *in_contact, const float *lamw, float inv_control_dt) {
  for (int j = 0; j < 12; j++) { r[j] = tq[j]; r[12 + j] = qd[j]; }
  for (int l = 0; l < 4; l++) { r[24 + l] = in_contact[l] != 0 ? 1.0f : 0.0f; r[28 + l] = irrl_eval_gait_fz(lamw[l * 3 + 2], inv_control_dt); }
}

// ---- the ensemble analysis of a body recorder: features, cell key, histogram bin (irrl_eval_ensemble, include/irrl_env.h) ----
// One recorder row (base x y z | quaternion w x y z | world linear velocity | world angular velocity) -> the reference's state vector
// x = (z, roll, pitch, body-frame v_z, body-frame w_x, body-frame w_y) (Data_Visualization_Code/Figure4.py:98-101), every word widened to f64 first,
// the rotation matrix and the angles as irrl_eval_env_epilogue builds them.  Element 3 is (R^T v)_z, NOT the statistics' world v_z.
static inline IRRL_EVAL_FN void irrl_eval_ensemble_features(const float *row13, double *x6) {
  const double pz = row13[2];
  const double w = row13[3], x = row13[4], y = row13[5], z = row13[6];
  const double v0 = row13[7], v1 = row13[8], v2 = row13[9];
  const double o0 = row13[10], o1 = row13[11], o2 = row13[12];
  const double r00 = 1 - 2 * (y * y + z * z), r01 = 2 * (x * y - w * z), r02 = 2 * (x * z + w * y);
  const double r10 = 2 * (x * y + w * z), r11 = 1 - 2 * (x * x + z * z), r12 = 2 * (y * z - w * x);
  const double r20 = 2 * (x * z - w * y), r21 = 2 * (w * x + y * z), r22 = 1 - 2 * (x * x + y * y);
  const double roll = atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y));
  double sp = 2 * (w * y - x * z);
  sp = sp > 1.0 ? 1.0 : sp < -1.0 ? -1.0 : sp;
  x6[0] = pz;
  x6[1] = roll;
  x6[2] = asin(sp);
  x6[3] = r02 * v0 + r12 * v1 + r22 * v2;
  x6[4] = r00 * o0 + r10 * o1 + r20 * o2;
  x6[5] = r01 * o0 + r11 * o1 + r21 * o2;
}
static inline IRRL_EVAL_FN bool irrl_eval_ensemble_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN and +-inf
// The cell key of one sample: per feature c_i = (long long)(min(max(x_i, lb_i), ub_i) / prec_i) -- a C cast, truncation toward zero like the
// reference's astype(int), so the cell around 0 is double width -- and with lo_i = (long long)(lb_i / prec_i), hi_i = (long long)(ub_i / prec_i),
// radix_i = hi_i - lo_i + 1 the key is the mixed-radix number of (c_i - lo_i), feature 0 the most significant digit.  -> false (sample dropped)
// where a feature is not finite.  The spec has passed irrl_eval_ensemble_spec_error: every quotient fits a long long, the key stays below 2^63.
static inline IRRL_EVAL_FN bool irrl_eval_ensemble_key(const double *x6, const irrl_eval_ensemble_spec &s, uint64_t *key) {
  uint64_t k = 0;
  for (int i = 0; i < IRRL_EVAL_ENSEMBLE_DIM; i++) {
    const double x = x6[i];
    if (!irrl_eval_ensemble_finite(x)) return false;
    const double clipped = fmin(fmax(x, s.lb[i]), s.ub[i]);
    const long long c = (long long)(clipped / s.prec[i]);
    const long long lo = (long long)(s.lb[i] / s.prec[i]), hi = (long long)(s.ub[i] / s.prec[i]);
    k = k * (uint64_t)(hi - lo + 1) + (uint64_t)(c - lo);
  }
  *key = k;
  return true;
}
// The histogram bin of one (unclipped) feature value, or -1: floor((x - lo) * (bins / (hi - lo))), x == hi in the last bin, outside [lo, hi]
// dropped.  (The product can round up to `bins` for an x one ulp under hi: that lands in the last bin too.)
static inline IRRL_EVAL_FN int irrl_eval_ensemble_bin(double x, double lo, double hi, int bins) {
  if (!(x >= lo && x <= hi)) return -1;
  if (x == hi) return bins - 1;
  const double scale = (double)bins / (hi - lo);
  const double d = x - lo;
  const int b = (int)floor(d * scale);
  return b < bins ? b : bins - 1;
}
// what is wrong with a spec, or NULL: the refusals of irrl_eval_ensemble that concern the spec alone (host code: the product of the cell ranges
// is taken exactly, in 128-bit integers)
static inline const char *irrl_eval_ensemble_spec_error(const irrl_eval_ensemble_spec &s) {
  const double cells_max = 4611686018427387904.0;   // 2^62
  unsigned __int128 product = 1;
  for (int i = 0; i < IRRL_EVAL_ENSEMBLE_DIM; i++) {
    if (!(s.prec[i] > 0.0) || !irrl_eval_ensemble_finite(s.prec[i])) return "prec_i > 0";
    if (!irrl_eval_ensemble_finite(s.lb[i]) || !irrl_eval_ensemble_finite(s.ub[i]) || s.lb[i] > s.ub[i]) return "lb_i <= ub_i, both finite";
    const double ql = s.lb[i] / s.prec[i], qh = s.ub[i] / s.prec[i];
    if (!(fabs(ql) < cells_max && fabs(qh) < cells_max)) return "a bound lies beyond 2^62 cells";
    const long long lo = (long long)ql, hi = (long long)qh;
    product *= (unsigned __int128)(hi - lo + 1);
    if (product >= ((unsigned __int128)1 << 63)) return "the product of the six cell ranges reaches 2^63: the key does not fit 64 bits";
  }
  if (s.hist_bins < 0 || s.hist_bins > IRRL_EVAL_ENSEMBLE_MAX_BINS) return "hist_bins lies in 0 .. 256";
  if (s.hist_bins > 0)
    for (int i = 0; i < IRRL_EVAL_ENSEMBLE_DIM; i++)
      if (!(s.hist_hi[i] > s.hist_lo[i]) || !irrl_eval_ensemble_finite(s.hist_hi[i]) || !irrl_eval_ensemble_finite(s.hist_lo[i]))
        return "hist_lo_i < hist_hi_i, both finite";
  return NULL;
}

// ---- the recurrence analysis of a body recorder: frame row, normalised state, squared distance, quantised level (irrl_eval_recurrence) ----
// What the reference's recurrence plot does with ONE robot's recording (Data_Visualization_Code/Figure4.py:495-509): the state vector of
// irrl_eval_ensemble_features per frame, centred and divided by a box, all pairwise Euclidean distances, quantised as min(floor(d / eps), steps).
// the recorder row of analysed frame i
static inline IRRL_EVAL_FN long long irrl_eval_recurrence_row(int frame_first, int frame_every, int i) {
  return (long long)frame_first + (long long)i * (long long)frame_every;
}
// u_k = (x_k - (lb_k + ub_k) / 2.0) / (ub_k - lb_k) (Figure4.py:502), written with stride `su` between the six words (the kernel keeps the
// states of a robot as [6][T] in LDS); -> false (frame dropped, nothing written) where a feature is not finite
static inline IRRL_EVAL_FN bool irrl_eval_recurrence_state(const double *x6, const irrl_eval_recurrence_spec &s, double *u, size_t su) {
  for (int k = 0; k < IRRL_EVAL_ENSEMBLE_DIM; k++)
    if (!irrl_eval_ensemble_finite(x6[k])) return false;
  for (int k = 0; k < IRRL_EVAL_ENSEMBLE_DIM; k++) {
    const double sum = s.lb[k] + s.ub[k];
    const double mid = sum / 2.0;
    const double width = s.ub[k] - s.lb[k];
    const double centred = x6[k] - mid;
    u[(size_t)k * su] = centred / width;
  }
  return true;
}
// d^2 = sum_k D_k D_k in index order, D_k = u_i[k] - u_j[k]; every product a statement of its own (no fused multiply-add).  si / sj: the
// strides between the six words of u_i / u_j.  The same bits with i and j exchanged (D_k changes its sign alone).
static inline IRRL_EVAL_FN double irrl_eval_recurrence_dist2(const double *ui, size_t si, const double *uj, size_t sj) {
  double d2 = 0.0;
  for (int k = 0; k < IRRL_EVAL_ENSEMBLE_DIM; k++) {
    const double delta = ui[(size_t)k * si] - uj[(size_t)k * sj];
    const double sq = delta * delta;
    d2 = d2 + sq;
  }
  return d2;
}
// q = c >= steps ? steps : (int)floor(c) with c = sqrt(d^2) / eps; a d^2 that is not a number (states that overflowed) gives `steps` too.
// Monotone in d^2: sqrt and the division are correctly rounded on host and device.
static inline IRRL_EVAL_FN int irrl_eval_recurrence_level(double d2, double eps, int steps) {
  const double d = sqrt(d2);
  const double c = d / eps;
  if (!(c < (double)steps)) return steps;
  return (int)floor(c);
}
// The smallest d^2 whose level reaches `radius` (+inf where none does): level(d2) < radius  <=>  d2 < threshold for every d2 >= 0, because the
// level is monotone.  Bisection over the bit patterns of the non-negative doubles, which are ordered like their values; host code, run once per
// call, so that the kernel decides R_ij without a square root and a division where nobody asks for q itself.
static inline double irrl_eval_recurrence_threshold(double eps, int steps, int radius) {
  uint64_t lo = 0, hi = 0x7FF0000000000000ull;               // level(0) = 0 < radius <= steps = level(+inf)
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    double d2;
    memcpy(&d2, &mid, sizeof d2);
    if (irrl_eval_recurrence_level(d2, eps, steps) < radius) lo = mid; else hi = mid;
  }
  double t;
  memcpy(&t, &hi, sizeof t);
  return t;
}
// what is wrong with a spec, or NULL: the refusals of irrl_eval_recurrence that concern the spec alone (matrix_env needs num_envs: the caller's)
static inline const char *irrl_eval_recurrence_spec_error(const irrl_eval_recurrence_spec &s) {
  for (int k = 0; k < IRRL_EVAL_ENSEMBLE_DIM; k++)
    if (!irrl_eval_ensemble_finite(s.lb[k]) || !irrl_eval_ensemble_finite(s.ub[k]) || !(s.ub[k] > s.lb[k])) return "lb_k < ub_k, both finite";
  if (!(s.eps > 0.0) || !irrl_eval_ensemble_finite(s.eps)) return "eps > 0, finite";
  if (s.steps < 1 || s.steps > 255) return "steps lies in 1 .. 255";
  if (s.radius < 1 || s.radius > s.steps) return "radius lies in 1 .. steps";
  if (s.theiler < 0 || s.lmin < 1 || s.vmin < 1) return "theiler >= 0, lmin >= 1, vmin >= 1";
  if (s.lags < 0) return "lags lies in 0 .. frames";
  if (s.matrix_count < 0 || s.matrix_count > IRRL_EVAL_RECURRENCE_MAX_MATRICES) return "matrix_count lies in 0 .. 8";
  return NULL;
}

// ---- the footfall analysis of a gait recorder: contact flag, dilation, hold, phase bin (irrl_eval_footfall, include/irrl_env.h) ----
// the raw contact flag of one recorder word (column 24 + leg of a rec_gait row): anything but zero, a NaN included
static inline IRRL_EVAL_FN bool irrl_eval_footfall_flag(float word) { return word != 0.0f; }
// THE FILTER RULE in its sequential, normative form: c[T] raw flags (0 / 1) of one leg over the robot's window -> f[T].
//   dilate: d[k] = any c[k'] with |k' - k| <= reach, 0 <= k' < T
//   hold:   f = d; in increasing j = 0 .. T - hold - 2: if f[j] && !f[j+1], f[j+1] = any of f[j+1 .. j+hold]
// reach = 2, hold = 10: Data_Visualization_Code/Figure2.py:97-116 for every T >= 5.
static inline IRRL_EVAL_FN void irrl_eval_footfall_filter(const uint8_t *c, int T, int reach, int hold, uint8_t *f) {
  for (int k = 0; k < T; k++) {
    const int k0 = k - reach < 0 ? 0 : k - reach;
    const int k1 = k + reach > T - 1 ? T - 1 : k + reach;
    uint8_t d = 0;
    for (int i = k0; i <= k1; i++)
      if (c[i] != 0) d = 1;
    f[k] = d;
  }
  for (int j = 0; j <= T - hold - 2; j++) {
    if (f[j] == 0 || f[j + 1] != 0) continue;
    uint8_t any = 0;
    for (int i = j + 1; i <= j + hold; i++)
      if (f[i] != 0) any = 1;
    f[j + 1] = any;
  }
}
// THE CLOSED FORM of the hold for one gap of d: a = the last frame in front of the gap with d (-1: none), b = the first frame behind it with d
// (>= T: none).  -> the frames a < k < end are filled, the frames end <= k < b are not: f[k] = k <= T - hold - 1 && b - a <= hold for the frames
// of the gap, so a gap of at most hold - 1 frames is filled up to the window's last `hold` frames, and a leading or trailing gap never.
static inline IRRL_EVAL_FN int irrl_eval_footfall_fill_end(int T, int hold, int a, int b) {
  if (a < 0 || b >= T || b - a > hold) return a + 1;
  const int last = T - hold;                               // the first frame the rule no longer reaches
  const int end = b < last ? b : last;
  return end > a + 1 ? end : a + 1;
}
// the phase bin of a touchdown at frame t inside the stride [a, b) of leg 0 (a <= t < b): (t - a) * bins / (b - a), integer division
static inline IRRL_EVAL_FN int irrl_eval_footfall_phase_bin(int t, int a, int b, int bins) { return (t - a) * bins / (b - a); }
// what is wrong with a spec, or NULL
static inline const char *irrl_eval_footfall_spec_error(const irrl_eval_footfall_spec &s) {
  if (s.reach < 0 || s.reach > IRRL_EVAL_FOOTFALL_MAX_REACH) return "reach lies in 0 .. 8";
  if (s.hold < 0 || s.hold > IRRL_EVAL_FOOTFALL_MAX_HOLD) return "hold lies in 0 .. 64";
  if (s.phase_bins < 0 || s.phase_bins > IRRL_EVAL_FOOTFALL_MAX_BINS) return "phase_bins lies in 0 .. 64";
  return NULL;
}

// ---- the motor plane of a gait recorder: sample, envelope, classes (irrl_eval_motor_plane, include/irrl_env.h) ----
// One recorder pair (joint torque, joint rate) of joint j -> motor-side torque m and speed w; -> false (sample dropped) unless both are finite
static inline IRRL_EVAL_FN bool irrl_eval_motor_sample(float tq, float qd, int j, double knee_ratio, double *m, double *w) {
  const double ratio = (j % 3 == 2) ? knee_ratio : 1.0;
  *m = (double)tq / ratio;
  *w = (double)qd * ratio;
  return irrl_eval_ensemble_finite(*m) && irrl_eval_ensemble_finite(*w);
}
// The upper envelope at motor speed w, the f64 restatement of the env's torque clamp (csrc/env_core.hpp torque_clamp1): tau_max up to w_crit,
// from there a straight line through zero at w_max.  Every product a statement of its own.  low(w) = -up(-w).
static inline IRRL_EVAL_FN double irrl_eval_motor_up(double w, const irrl_eval_motor_spec &s) {
  if (!(w > s.w_crit)) return s.tau_max;
  const double span = s.w_max - s.w_crit;
  const double slope = s.tau_max / span;
  const double over = w - s.w_crit;
  const double drop = over * slope;
  return s.tau_max - drop;
}
static inline IRRL_EVAL_FN double irrl_eval_motor_low(double w, const irrl_eval_motor_spec &s) { return -irrl_eval_motor_up(-w, s); }
// the classes of one kept sample as bits: 1 SAT_UP, 2 SAT_LOW, 4 OUTSIDE, 8 MOTORING, 16 BRAKING (bit k = counter k + 1)
static inline IRRL_EVAL_FN unsigned irrl_eval_motor_classes(double m, double w, const irrl_eval_motor_spec &s) {
  const double up = irrl_eval_motor_up(w, s), low = irrl_eval_motor_low(w, s);
  const double up_in = up - s.sat, up_out = up + s.sat;
  const double low_in = low + s.sat, low_out = low - s.sat;
  const double power = m * w;
  unsigned bits = 0u;
  if (m >= up_in) bits |= 1u;
  if (m <= low_in) bits |= 2u;
  if (m > up_out || m < low_out) bits |= 4u;
  if (power > 0.0) bits |= 8u;
  if (power < 0.0) bits |= 16u;
  return bits;
}
// what is wrong with a spec, or NULL
static inline const char *irrl_eval_motor_spec_error(const irrl_eval_motor_spec &s) {
  if (!irrl_eval_ensemble_finite(s.tau_max) || !(s.tau_max > 0.0)) return "tau_max > 0, finite";
  if (!irrl_eval_ensemble_finite(s.w_crit) || !irrl_eval_ensemble_finite(s.w_max) || !(s.w_max > s.w_crit)) return "w_crit < w_max, both finite";
  if (!irrl_eval_ensemble_finite(s.knee_ratio) || !(s.knee_ratio > 0.0)) return "knee_ratio > 0, finite";
  if (!irrl_eval_ensemble_finite(s.sat) || !(s.sat >= 0.0)) return "sat >= 0, finite";
  if (s.t_bins < 0 || s.t_bins > IRRL_EVAL_MOTOR_MAX_BINS || s.w_bins < 0 || s.w_bins > IRRL_EVAL_MOTOR_MAX_BINS) return "t_bins, w_bins lie in 0 .. 64";
  if (s.period < 0 || s.period > IRRL_EVAL_MOTOR_MAX_PERIOD) return "period lies in 0 .. 1024";
  if (s.t_bins > 0 && s.w_bins > 0) {
    if (!irrl_eval_ensemble_finite(s.t_lo) || !irrl_eval_ensemble_finite(s.t_hi) || !(s.t_hi > s.t_lo)) return "t_lo < t_hi, both finite";
    if (!irrl_eval_ensemble_finite(s.w_lo) || !irrl_eval_ensemble_finite(s.w_hi) || !(s.w_hi > s.w_lo)) return "w_lo < w_hi, both finite";
  }
  return NULL;
}

// ---- the correlation moments of two recorder windows (irrl_eval_correlation, include/irrl_env.h) ----
// THE accumulation: s + (double)a * (double)b.  The product of two f32 values has at most 48 significant bits and is exact in f64, so the fused
// form (one rounding of s + a b) and the separate form (an exact product, one rounding of the sum) are the same number: host compiler, device
// compiler and numpy agree bit for bit as long as every accumulator takes its samples in the one stated order.  sum x is b = 1, sum x^2 is b = a.
static inline IRRL_EVAL_FN double irrl_eval_corr_add(double s, float a, float b) { return s + (double)a * (double)b; }
// the running minimum / maximum: m unless v is smaller / larger -- a NaN never enters a range
static inline IRRL_EVAL_FN float irrl_eval_corr_min(float m, float v) { return v < m ? v : m; }
static inline IRRL_EVAL_FN float irrl_eval_corr_max(float m, float v) { return v > m ? v : m; }
// the f64 accumulators of one robot: sxy [cx, cy] | sx [cx, 2] | sy [cy, 2]
static inline IRRL_EVAL_FN size_t irrl_eval_corr_sums(const irrl_eval_corr_spec &s) {
  return (size_t)s.x_count * (size_t)s.y_count + 2 * (size_t)s.x_count + 2 * (size_t)s.y_count;
}
// the doubles of `work` per robot: the sums, T_e as an int64, the two ranges as f32 pairs
static inline IRRL_EVAL_FN size_t irrl_eval_corr_work_per_env(const irrl_eval_corr_spec &s) {
  return irrl_eval_corr_sums(s) + 1 + (size_t)s.x_count + (size_t)s.y_count;
}
// what is wrong with a spec, or NULL
static inline const char *irrl_eval_corr_spec_error(const irrl_eval_corr_spec &s) {
  if (s.x_dim < 1 || s.y_dim < 1) return "x_dim >= 1, y_dim >= 1";
  if (s.x_count < 1 || s.x_count > IRRL_EVAL_CORR_MAX_X) return "x_count lies in 1 .. 64";
  if (s.y_count < 1 || s.y_count > IRRL_EVAL_CORR_MAX_Y) return "y_count lies in 1 .. 1024";
  if (s.x_first < 0 || (long long)s.x_first + (long long)s.x_count > (long long)s.x_dim) return "the x window x_first .. x_first + x_count lies outside the row width x_dim";
  if (s.y_first < 0 || (long long)s.y_first + (long long)s.y_count > (long long)s.y_dim) return "the y window y_first .. y_first + y_count lies outside the row width y_dim";
  return NULL;
}

// ---- the spectrogram and the Welch spectrum of recorder columns (irrl_eval_spectrum, include/irrl_env.h) ----
// scipy.signal.spectrogram(mode='psd', scaling='density', return_onesided=True, nfft=nperseg) as a direct DFT, every step in f64.  The steps that
// are a product next to a sum are statements of their own, so that no compiler fuses them (the library is built with -ffp-contract=on) -- all
// but THE accumulation, irrl_eval_spectrum_add, which is written as one expression: the device fuses it, a host without a fused multiply-add
// does not, and the tests' bound (n 2^-53 sum |a_n| per dot product, in any order, fused or not) covers both.
static inline IRRL_EVAL_FN int irrl_eval_spectrum_bins(int nperseg) { return nperseg / 2 + 1; }
// S_e: the segments s * hop .. s * hop + nperseg - 1 that lie wholly inside the frames i < T_e
static inline IRRL_EVAL_FN int irrl_eval_spectrum_segments(int te, int nperseg, int hop) { return te >= nperseg ? (te - nperseg) / hop + 1 : 0; }
// v_n = (double)x_n * scale[c]
static inline IRRL_EVAL_FN double irrl_eval_spectrum_sample(float x, double scale) { return (double)x * scale; }
// m = (((zero + v_0) + v_1) + ...) / nperseg over the words v[0], v[stride], ...; zero is +0.0 (why it is an argument: eval_correlation.hip)
static inline IRRL_EVAL_FN double irrl_eval_spectrum_mean(const double *v, size_t stride, int nperseg, double zero) {
  double t = zero;
  for (int n = 0; n < nperseg; n++) t = t + v[(size_t)n * stride];
  return t / (double)nperseg;
}
// a_n = (v_n - m) * window[n]; without a detrend nothing is subtracted (not even 0.0: -0.0 stays what it is)
static inline IRRL_EVAL_FN double irrl_eval_spectrum_windowed(double v, double m, int detrend, double w) {
  const double d = detrend ? v - m : v;
  return d * w;
}
// THE accumulation of Re_k (t = cos) and of -Im_k (t = sin): s + a * t, n ascending
static inline IRRL_EVAL_FN double irrl_eval_spectrum_add(double s, double a, double t) { return s + a * t; }
// the next (k n) mod nperseg out of the last, 0 <= k < nperseg
static inline IRRL_EVAL_FN int irrl_eval_spectrum_step(int j, int k, int nperseg) {
  const int next = j + k;
  return next >= nperseg ? next - nperseg : next;
}
// g_k: 2, except g_0 = 1 and, with an even nperseg, g_{K-1} = 1 (the bins without a mirror image)
static inline IRRL_EVAL_FN double irrl_eval_spectrum_gain(int k, int nperseg) { return (k == 0 || 2 * k == nperseg) ? 1.0 : 2.0; }
// P_k = g_k * density * (Re_k^2 + Im_k^2) with Im_k = -sim, the negated sum of the sines
static inline IRRL_EVAL_FN double irrl_eval_spectrum_power(double re, double sim, double gain, double density) {
  const double im = -sim;
  const double re2 = re * re;
  const double im2 = im * im;
  const double mag2 = re2 + im2;
  const double f = gain * density;
  return f * mag2;
}
// density = 1 / (fs * sum_n window[n]^2), the squares added in ascending order from zero = +0.0 (a square is never -0.0: the argument is there
// for the rule's sake); once per workgroup on the device, the window is the caller's device table
static inline IRRL_EVAL_FN double irrl_eval_spectrum_density(const double *window, int nperseg, double fs, double zero) {
  double t = zero;
  for (int n = 0; n < nperseg; n++) {
    const double sq = window[n] * window[n];
    t = t + sq;
  }
  const double d = fs * t;
  return 1.0 / d;
}
// the doubles of `work` per robot: the partials [cx, K] and S_e as an int64
static inline IRRL_EVAL_FN size_t irrl_eval_spectrum_work_per_env(const irrl_eval_spectrum_spec &s) {
  return (size_t)s.x_count * (size_t)irrl_eval_spectrum_bins(s.nperseg) + 1;
}
// what is wrong with a spec, or NULL (the matrix_env range needs num_envs: the call checks it)
static inline const char *irrl_eval_spectrum_spec_error(const irrl_eval_spectrum_spec &s) {
  if (s.x_dim < 1) return "x_dim >= 1";
  if (s.x_count < 1 || s.x_count > IRRL_EVAL_SPECTRUM_MAX_X) return "x_count lies in 1 .. 64";
  if (s.x_first < 0 || (long long)s.x_first + (long long)s.x_count > (long long)s.x_dim) return "the x window x_first .. x_first + x_count lies outside the row width x_dim";
  if (s.nperseg < 8 || s.nperseg > IRRL_EVAL_SPECTRUM_MAX_NPERSEG) return "nperseg lies in 8 .. 1024";
  if (s.hop < 1 || s.hop > s.nperseg) return "hop lies in 1 .. nperseg";
  if (s.detrend < 0 || s.detrend > 1) return "detrend lies in 0 .. 1";
  if (!irrl_eval_ensemble_finite(s.fs) || !(s.fs > 0.0)) return "fs > 0, finite";
  for (int c = 0; c < s.x_count; c++)
    if (!irrl_eval_ensemble_finite(s.scale[c]) || !(s.scale[c] > 0.0)) return "scale_c > 0, finite, for every analysed column";
  if (s.matrix_count < 0 || s.matrix_count > IRRL_EVAL_SPECTRUM_MAX_MATRICES) return "matrix_count lies in 0 .. 8";
  return NULL;
}
// what is wrong with the arguments of irrl_eval_spectrum_tables, or NULL
static inline const char *irrl_eval_spectrum_tables_error(int nperseg, int window_kind, double alpha, const double *window, const double *tw) {
  if (!window || !tw) return "NULL window or tw";
  if (nperseg < 8 || nperseg > IRRL_EVAL_SPECTRUM_MAX_NPERSEG) return "nperseg lies in 8 .. 1024";
  if (window_kind < 0 || window_kind > 2) return "window_kind lies in 0 .. 2 (boxcar, Hann, Tukey)";
  if (!irrl_eval_ensemble_finite(alpha)) return "alpha is finite";
  return NULL;
}
// The tables of irrl_eval_spectrum_tables (include/irrl_env.h states the formulas against scipy's): window [nperseg], tw [nperseg, 2].  Host code.
static inline void irrl_eval_spectrum_tables_fill(int nperseg, int window_kind, double alpha, double *window, double *tw) {
  const double pi = 3.14159265358979323846;
  if (window_kind == 2 && alpha <= 0.0) window_kind = 0;
  if (window_kind == 2 && alpha >= 1.0) window_kind = 1;
  const int M = nperseg + 1;                                   // the periodic window: the symmetric one of M samples without its last
  const int width = window_kind == 2 ? (int)floor(alpha * (double)(M - 1) / 2.0) : 0;
  for (int n = 0; n < nperseg; n++) {
    double w = 1.0;
    if (window_kind == 1) {
      w = 0.5 - 0.5 * cos(2.0 * pi * (double)n / (double)nperseg);
    } else if (window_kind == 2) {
      if (n <= width) w = 0.5 * (1.0 + cos(pi * (-1.0 + 2.0 * (double)n / alpha / (double)(M - 1))));
      else if (n >= M - width - 1) w = 0.5 * (1.0 + cos(pi * (-2.0 / alpha + 1.0 + 2.0 * (double)n / alpha / (double)(M - 1))));
    }
    window[n] = w;
    const double phi = 2.0 * pi * (double)n / (double)nperseg;
    tw[2 * n] = cos(phi);
    tw[2 * n + 1] = sin(phi);
  }
}
