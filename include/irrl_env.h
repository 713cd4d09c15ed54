/*
 * irrl_env.h -- C-ABI of the MI355X-native BlackPanther vector environment (libirrl_env.so).
 *
 * This is the drop-in boundary for the hot path  FlexibleGymEnv.step()  of
 * WoodenJin/High_Speed_Quadrupedal_Locomotion_by_IRRL.  Every entry point names the reference
 * interface it replaces; paths are under IRRL/FlexibleRobotRaisimGym/flex_gym/env/ :
 *   PYB = raisim_gym.cpp (pybind11 module `_flexible_robot`, class `FlexibleGymEnv`)
 *   VEC = VectorizedEnvironment.hpp,  ENV = env/BlackPanther_V55/Environment.hpp
 *
 * Conventions
 *   - plain C: opaque handle, pointers and sizes only; no torch / pybind / Eigen types.
 *   - every function returns 0 on success, non-zero on failure (irrl_last_error() has the text);
 *     the reference has no error channel: it aborts on a missing YAML key (RaisimGymEnv.hpp:41-42).
 *   - "device pointer" entry points (suffix-less) take HIP device pointers and are stream-ordered on the
 *     stream given to irrl_env_set_stream (default: the null stream); they never synchronise.
 *     "_host" entry points take host pointers like the reference's numpy arrays
 *     (Eigen::Ref<RowMajor float/bool>, RaisimGymEnv.hpp:46-49), copy through a pinned staging buffer and
 *     return after the outputs are valid on the host.
 *   - the library needs a gfx950 GPU: irrl_env_create fails (returns NULL) when none is usable.
 *     There is no CPU fallback of any kind behind this ABI.
 *   - array shapes: ob [N,35] f32, action [N,12] f32, reward [N] f32, done [N] u8 (numpy bool),
 *     extraInfo [N,6] f32, all C-contiguous, caller-owned, written in place (RaisimGymVecEnv.py:16-20).
 */
#ifndef IRRL_ENV_H
#define IRRL_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct irrl_env irrl_env;

#define IRRL_OB_DIM 35      /* ENV:360 */
#define IRRL_ACTION_DIM 12  /* ENV:361 */
#define IRRL_EXTRA_DIM 6    /* ENV:942-950 */
#define IRRL_ORIGIN_STATE_DIM 41 /* ENV:1330-1334: gc 19 + gv 18 + contact 4 */

const char *irrl_last_error(void);
/* build identification: "gfx950;<git-describe or date>" */
const char *irrl_version(void);

/* PYB:16 ctor (std::string resourceDir, std::string cfg) -> VEC:132-138.  cfg_yaml is the dumped
 * `environment:` mapping (run_bp_v5.py:205-207).  device = HIP device ordinal.  NULL on failure. */
irrl_env *irrl_env_create(const char *resource_dir, const char *cfg_yaml, int device);
/* VEC:140-143 destructor */
void irrl_env_destroy(irrl_env *h);
/* PYB:17 init -> VEC:145-194 (constructor randomisation ENV:435-477 + first reset of every env) */
int irrl_env_init(irrl_env *h);
/* use `hip_stream` (a hipStream_t) for all later launches / async copies of this handle */
int irrl_env_set_stream(irrl_env *h, void *hip_stream);

/* PYB:28-31 */
int irrl_env_num_envs(const irrl_env *h);
/* lane layout of this pool's kernels: 16 (one DPP row per robot: while the pool's waves of four robots fit the device's SIMDs, <= 4096 envs
 * on an MI355X) or 4 (larger pools: one DPP quad per robot); build-defined, overridable with the environment variable IRRL_LANES_PER_ROBOT */
int irrl_env_lanes_per_robot(const irrl_env *h);
/* resident waves per SIMD the pool's kernels are compiled for: 1 (the whole register file of a SIMD for one wave), or 2 for 4-lane pools
 * with more waves than the device has SIMDs (> 16 384 envs on an MI355X); build-defined, overridable with IRRL_L4_WAVES=1|2 */
int irrl_env_waves_per_simd(const irrl_env *h);
/* WHICH KERNELS A CONFIGURATION SELECTS.  The step kernel exists in six variants and the settings alone decide which one a pool runs:
 *   "crutial" / "crutial_md"  Crutial: True (the meteorite), first / published per-contact rule
 *   "dir"                     ContactSolver 0 or 2: the build's first per-contact rule
 *   "md"                      the published rule (ContactSolver 1 or 3) with the solver settings read at run time
 *   "shipped" / "shipped_flat"  the published rule with the shipped settings compiled in -- ContactSolver 3, ContactExit 1, ContactTolerance > 0,
 *                             ContactIterations 6, eight substeps per control step -- on rough / flat ground
 * irrl_kernel_variant_for is a function of the settings alone (host only, no device needed): contact_solver / contact_exit / contact_tol /
 * contact_iters are the Contact* keys as resolved by the parser (absent keys: 3 / 1 / 0.0 / 6 -- so a config WITHOUT ContactTolerance is "md"),
 * substeps = control_dt / simulation_dt, terrain = Terrain.  "" for a contact_solver outside 0..3.  The strings are stable. */
const char *irrl_kernel_variant_for(int crutial, int contact_solver, int contact_exit, double contact_tol, int contact_iters, int substeps, int terrain);
/* the pool's variant right now (read per call: irrl_env_set_control_dt / irrl_env_set_simulation_dt change the substep count) */
const char *irrl_env_kernel_variant(const irrl_env *h);
/* name of the kernel that irrl_env_step (path 0) or irrl_env_step_rows_persistent[_out] (path 1) launches for this pool right now, lane-layout
 * suffix included (e.g. "irrl_steps_persistent_kernel_rt_l16"); where path 1 falls back to one launch per step, the step kernel's name.
 * "" for any other path. */
const char *irrl_env_kernel_name(const irrl_env *h, int path);
/* 1: irrl_env_step_rows_persistent[_out] run as ONE launch for this pool, 0: they fall back to one launch per step (Crutial pools), -1: NULL handle */
int irrl_env_persistent_supported(const irrl_env *h);
int irrl_env_ob_dim(const irrl_env *h);
int irrl_env_action_dim(const irrl_env *h);
int irrl_env_extra_dim(const irrl_env *h);
/* PYB:18 getExtraInfoNames (VEC:191-193): name j in [0, 6); order fixed by this build */
const char *irrl_env_extra_name(const irrl_env *h, int j);

/* PYB:21,23 step -> VEC:268-278 (+ perAgentStep VEC:352-372, ENVIRONMENT::step ENV:692-809) */
int irrl_env_step(irrl_env *h, const float *action, float *ob, float *reward, uint8_t *done, float *extra);
int irrl_env_step_host(irrl_env *h, const float *action, float *ob, float *reward, uint8_t *done, float *extra);
/* build-defined: `count` consecutive steps from a device-resident action table [n_rows, N, 12] (step k takes row
 * (first_row + k) % n_rows), launched back to back on the env's stream by one call -- open-loop playback / benchmarking without a
 * host round trip per step.  Outputs as irrl_env_step: [N, .] arrays that every step overwrites (those of the last step survive). */
int irrl_env_step_rows(irrl_env *h, int count, const float *action_rows, int n_rows, int first_row, float *ob, float *reward,
                       uint8_t *done, float *extra);
/* the same `count` steps as ONE launch: a wave walks its own robots through all of them (robots never interact, VEC:273), so there is no
 * grid-wide boundary between steps and no launch per step.  States and outputs bit-identical to irrl_env_step_rows.  Every pool WITHOUT the
 * meteorite gets the single launch, whatever its contact rule, solver settings or substep count (kernel variants "dir", "md", "shipped",
 * "shipped_flat"; all three lane layouts); Crutial pools fall back to irrl_env_step_rows.  irrl_env_persistent_supported tells which. */
int irrl_env_step_rows_persistent(irrl_env *h, int count, const float *action_rows, int n_rows, int first_row, float *ob, float *reward,
                                  uint8_t *done, float *extra);
/* the two calls above WITH EVERY STEP'S OUTPUTS KEPT: ob_rows [count, N, 35], reward_rows [count, N], done_rows [count, N] u8,
 * extra_rows [count, N, 6] (device); step k fills row k -- exactly what `count` calls of the reference's step() hand back one after the
 * other (VEC:268-278 fills ob / reward / done / extraInfo on every control step; RaisimGymVecEnv.py:26-52 copies them out), so the caller
 * of the K-step entry point gets the trajectory it simulated.  Rows bit-identical to `count` irrl_env_step calls. */
int irrl_env_step_rows_out(irrl_env *h, int count, const float *action_rows, int n_rows, int first_row, float *ob_rows, float *reward_rows,
                           uint8_t *done_rows, float *extra_rows);
int irrl_env_step_rows_persistent_out(irrl_env *h, int count, const float *action_rows, int n_rows, int first_row, float *ob_rows,
                                      float *reward_rows, uint8_t *done_rows, float *extra_rows);
/* PYB:24 testStep -> VEC:280-290: env 0 only in the reference (visual eval); here it steps env 0 only and
 * leaves rows 1.. of the outputs untouched (headless: no rendering). */
int irrl_env_test_step_host(irrl_env *h, const float *action, float *ob, float *reward, uint8_t *done, float *extra);
/* PYB:19 reset -> VEC:201-207 (all envs, then observe) */
int irrl_env_reset(irrl_env *h, float *ob);
int irrl_env_reset_host(irrl_env *h, float *ob);
/* PYB:20 observe -> VEC:209-212 */
int irrl_env_observe(irrl_env *h, float *ob);
int irrl_env_observe_host(irrl_env *h, float *ob);
/* PYB:26 isTerminalState -> VEC:314-319 */
int irrl_env_is_terminal(irrl_env *h, uint8_t *done);
int irrl_env_is_terminal_host(irrl_env *h, uint8_t *done);
/* PYB:22 setSeed -> VEC:308-312.  The reference seeds the process-global std::srand per env
 * (last call wins); here it re-keys the counter RNG for all later draws. */
int irrl_env_set_seed(irrl_env *h, int seed);
/* PYB:27-28 setSimulationTimeStep / setControlTimeStep -> VEC:321-329 */
int irrl_env_set_simulation_dt(irrl_env *h, double dt);
int irrl_env_set_control_dt(irrl_env *h, double dt);
/* PYB:25 close (no-op, ENV:1585), PYB:36 curriculumUpdate (no-op, RaisimGymEnv.hpp:76) */
int irrl_env_close(irrl_env *h);
int irrl_env_curriculum_update(irrl_env *h);

/* diagnostics getters, host pointers (PYB:37-45; RaisimGymVecEnv.py:54-93) */
int irrl_env_origin_state_host(irrl_env *h, float *out /* [N,41]  ENV:1317-1325 */);
int irrl_env_reference_state_host(irrl_env *h, float *out /* [N,24] ENV:1339-1345 jointRef, jointDotRef */);
int irrl_env_joint_effort_host(irrl_env *h, float *out /* [N,12] ENV:1350-1358 */);
int irrl_env_generalized_force_host(irrl_env *h, float *out /* [N,18] ENV:1363-1370 */);
int irrl_env_inverse_mass_matrix_host(irrl_env *h, float *out /* [N,324] column-major, ENV:1375-1391 */);
int irrl_env_nonlinear_host(irrl_env *h, float *out /* [N,18] ENV:1396-1402 */);
int irrl_env_set_contact_coeff_host(irrl_env *h, const float *in /* [N,3] mu, e, thr; ENV:1407-1418 */);
/* PYB:46 / VEC:253-256 GetSphereInfo (ENV:1423-1436): centre (world) and radius of the meteorite of a `Crutial: True` pool;
 * an error on a pool without it (the reference prints "Please make sure the [Flag_Crucial] is True") */
int irrl_env_sphere_info_host(irrl_env *h, float *out /* [N,4] */);

/* Full state exchange (build-defined, for checkpoint/parity): flat [N, IRRL_STATE_DIM] doubles per env,
 * fields at the IRRL_S_* offsets below. */
#define IRRL_STATE_DIM 288
enum {
  IRRL_S_GC = 0, IRRL_S_GV = 19, IRRL_S_PTARGET_LAST = 37, IRRL_S_TORQUE_LAST = 49, IRRL_S_TORQUE = 61,
  IRRL_S_JOINT_REF = 73, IRRL_S_JOINT_REF_LAST = 85, IRRL_S_JOINT_DOT_REF = 97, IRRL_S_EE_REF = 109,
  IRRL_S_COMMAND = 121, IRRL_S_COMMAND_FILTERED = 124, IRRL_S_T0 = 127, IRRL_S_FRAME = 128, IRRL_S_EPISODE = 129,
  IRRL_S_UP_HEIGHT = 130, IRRL_S_CONTACT = 131, IRRL_S_LAMBDA_W = 135, IRRL_S_IN_CONTACT = 147,
  IRRL_S_MATERIAL = 151, IRRL_S_MASS = 154, IRRL_S_COM = 167, IRRL_S_THIGH_DZ = 206, IRRL_S_OB = 207,
  IRRL_S_OB_LAST = 242,
  IRRL_S_SPHERE = 277 /* Crutial: meteorite centre 3, velocity 3, radius, mass, body type (0 static / 1 dynamic) */, IRRL_S_END = 286
};
int irrl_env_get_state_host(irrl_env *h, double *out);
int irrl_env_set_state_host(irrl_env *h, const double *in);
/* ENV:1895 set_ref / VEC:158-176: the reference-trajectory table of a `ManualTraj: False` pool, [rows, cols >= 30] row-major
 * f32 (theta 12 | theta_dot 12 | z | phase 2 | cmd 3 per control step, Environment.hpp:17-21).  create() loads the CSV named
 * by cfg["RefTraj"] when it is readable (VectorizedEnvironment.hpp:33-76 format); otherwise call this before init(). */
int irrl_env_set_ref_host(irrl_env *h, const float *table, int rows, int cols);
/* the shared height field of a `Terrain: True` pool (Environment.hpp:254-264), [nx, ny] row-major f32; out may be NULL
 * to query the shape only; returns non-zero on flat ground */
int irrl_env_heightfield_host(irrl_env *h, float *out, int *nx, int *ny);
/* device-side snapshot of the whole state pool / its restoration, stream-ordered on the pool's stream: a caller can run
 * throw-away steps (the warm-up in front of a hipGraph capture of the rollout) and continue from where it was */
int irrl_env_snapshot(irrl_env *h);
int irrl_env_restore(irrl_env *h);
/* diagnostic counters summed over the pool (the role of the per-env members itera / contact list sizes a reference user would
 * print, Environment.hpp:554, 1199-1243): out[0] = episodes started (init + every reset), out[1] = toe-substeps spent in the
 * contact list since create(), out[2] = sum of frame_idx.  Synchronises the pool's stream.  bench.py differences them around
 * its timed region to show the region was not free flight. */
int irrl_env_counters_host(irrl_env *h, unsigned long long *out);
/* the same three sums written to d_out[3] (device memory), stream-ordered on the pool's stream, no synchronisation */
int irrl_env_counters(irrl_env *h, unsigned long long *d_out);
/* value of a numeric/bool config key as parsed by the library (tests the YAML reader); NaN if absent */
double irrl_env_cfg_value(const irrl_env *h, const char *key);

/* ---- learner-side device ops on the same path (ppo2.py:554-568): GAE reverse scan ---- */
/* rewards/values/adv/returns [T,N] f32 row-major, dones [T,N] u8 (flag stored BEFORE step t, ppo2.py:526),
 * last_values [N], last_dones [N]; device pointers, stream-ordered on `hip_stream`. */
int irrl_gae(int T, int N, const float *rewards, const float *values, const uint8_t *dones, const float *last_values,
             const uint8_t *last_dones, float gamma, float lam, float *adv, float *returns, void *hip_stream);

/* PPO2 clipped-surrogate loss of a diagonal-Gaussian policy, forward and backward in one pass (ppo2.py:152-175): M samples,
 * mean / actions [M, act], logstd [act], vpred / returns / old_values / old_neglogp [M], adv_stats = (mean, std) of the raw
 * advantages returns - old_values (device; all-reduced first when there are several ranks).  Writes d loss / d mean [M, act] and
 * d loss / d vpred [M] (loss = pg - ent_coef * entropy + vf_coef * vf; the constant entropy term is the caller's) and per-block
 * partial sums [n_blocks, 4 + act] = pg loss, vf loss, approx KL, clip fraction, d loss / d logstd (pg part); act = 12. */
int irrl_ppo_loss(size_t M, int act_dim, const float *mean, const float *logstd, const float *vpred, const float *actions,
                  const float *returns, const float *old_values, const float *old_neglogp, const float *adv_stats, float cliprange,
                  float vf_coef, float *d_mean, float *d_vpred, float *partials, int n_blocks, void *hip_stream);

/* the policy / value heads of CustomLSTMPolicy (run_bp_v5.py:169-176: mean = h_pi W_pi + b_pi, v = h_v w_v + b_v) TOGETHER with the
 * loss above, forward and backward in one pass: h_pi / h_v [M, hid] are the two stacks' last-layer outputs over the rollout.
 * Writes d loss / d h_pi, d loss / d h_v [M, hid] (and, if not NULL, mean [M, act] / value [M]) and per-block partial sums
 * [n_blocks, 4 + act + act + 1 + hid + hid * act] = (pg, vf, kl, clipfrac) | d logstd | d b_pi | d b_v | d w_v | d W_pi [hid][act].
 * hid = 48, act = 12. */
int irrl_ppo_heads_loss(size_t M, int act_dim, int hid, const float *h_pi, const float *h_v, const float *pi_w, const float *pi_b, const float *vf_w,
                        const float *vf_b, const float *logstd, const float *actions, const float *returns, const float *old_values,
                        const float *old_neglogp, const float *adv_stats, float cliprange, float vf_coef, float *d_hpi, float *d_hv, float *mean_out,
                        float *value_out, float *partials, int n_blocks, void *hip_stream);

/* MlpPolicy (archi/policies.py:430-446: [64, 64] tanh stacks for policy and value over the 35 observations; the learner of BASELINE
 * config 2) under the PPO2 loss above: forward AND backward of one network over one minibatch in one launch -- what ppo2.py:243-298
 * (`_train_step`) evaluates through the TensorFlow graph.  kind 0 = policy network (w3 [64, 12]; uses actions, old_neglogp, logstd and
 * the normalised advantages), kind 1 = value network (w3 [64, 1]; clipped value loss times vf_coef).  idx [n] (int64, device) selects
 * the minibatch's rows of the flat rollout arrays (NULL: rows 0..n-1); nothing is gathered.  Weights are [in, out] row-major.
 * Writes per-workgroup partial sums [n_blocks, irrl_mlp_ppo_partial_len()], to be added up by the caller (fixed order); a row is
 * scalars[4] (kind 0: pg loss, approx KL, clip fraction; kind 1: value loss -- sums over samples, divide by n) | d logstd[16] (pg part) |
 * d b1[64] | d b2[64] | d b3[16] | d W1[48][64] (rows >= 35 are zero) | d W2[64][64] | d W3[64][16] (columns >= act / 1 are zero),
 * gradients of loss = pg - ent_coef * entropy + vf_coef * vf with the means taken over the n samples. */
int irrl_mlp_ppo_grads(int kind, size_t n, const int64_t *idx, int ob_dim, int hid, int act_dim, const float *obs, const float *actions,
                       const float *returns, const float *old_values, const float *old_neglogp, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *w3, const float *b3, const float *logstd, const float *adv_stats, float cliprange, float vf_coef,
                       float *partials, int n_blocks, void *hip_stream);
int irrl_mlp_ppo_partial_len(void);
/* The same gradients with every matrix product formed as THREE bf16 plane products on the matrix cores (each operand split into two
 * bf16 planes, f32 accumulation: ~2^-16 relative per product, csrc/mlp_bf16.hpp): same arguments, same partial-sum rows, ~3x faster.
 * What the learner uses by default; irrl_mlp_ppo_grads stays the exact-f32 form. */
int irrl_mlp_ppo_grads_bf16(int kind, size_t n, const int64_t *idx, int ob_dim, int hid, int act_dim, const float *obs, const float *actions,
                            const float *returns, const float *old_values, const float *old_neglogp, const float *w1, const float *b1, const float *w2,
                            const float *b2, const float *w3, const float *b3, const float *logstd, const float *adv_stats, float cliprange, float vf_coef,
                            float *partials, int n_blocks, void *hip_stream);

/* PACKED SAMPLE RECORDS (round 5).  A minibatch row is a random sample of the flat rollout (ppo2.py:364-380), so each of the five arrays above
 * costs whole 128-byte lines per sample (3.8x / 3.3x the payload, PMC).  irrl_mlp_pack_records builds, once per update, one 256-byte record per
 * sample -- rec [n, irrl_mlp_record_floats() = 64]: words [0, 35) observation | [36, 48) action | 48 return | 49 old value | 50 old neglogp |
 * 51 return - old value | the rest zero; rec 256-byte aligned -- and irrl_mlp_ppo_grads_bf16_rec / irrl_adv_moments_rec read the minibatch's rows
 * out of it: two lines per sample, same values, bit-identical results. */
int irrl_mlp_pack_records(size_t n, const float *obs, const float *actions, const float *returns, const float *old_values, const float *old_neglogp,
                          float *rec, void *hip_stream);
int irrl_mlp_record_floats(void);
int irrl_mlp_ppo_grads_bf16_rec(int kind, size_t n, const int64_t *idx, const float *rec, const float *w1, const float *b1, const float *w2,
                                const float *b2, const float *w3, const float *b3, const float *logstd, const float *adv_stats, float cliprange,
                                float vf_coef, float *partials, int n_blocks, void *hip_stream);
int irrl_adv_moments_rec(size_t n, const int64_t *idx, const float *rec, double *scratch, int n_blocks, double *sums, float *stats, void *hip_stream);

/* moments of the raw advantages a = returns[r] - old_values[r] of one minibatch (ppo2.py:262-263 normalises them per minibatch):
 * sums[3] = (sum a, sum a^2, n) as doubles, rows through idx [n] (int64, device) or 0..n-1 (NULL), fixed summation order.
 * old_values may be NULL: `returns` then holds the advantages themselves (formed once per update: one gathered array per minibatch instead of two).
 * scratch: 2 * n_blocks doubles (device).  stats (device, may be NULL): also (mean, population std) of a as two floats -- the adv_stats
 * argument of the loss kernels when the job has one rank (several ranks all-reduce `sums` first). */
int irrl_adv_moments(size_t n, const int64_t *idx, const float *returns, const float *old_values, double *scratch, int n_blocks, double *sums,
                     float *stats, void *hip_stream);

/* ---- tail of one PPO2 optimizer step on FLAT buffers (ppo2.py:182-197: tf.clip_by_global_norm(max_grad_norm) then
 * tf.train.AdamOptimizer(lr, epsilon).apply_gradients; kernels csrc/ppo_optim.hpp).  theta / grad / m / v: [n] floats (device,
 * 16-byte aligned), the parameters, their gradient and the Adam moments; every parameter tensor of the policy is a view of theta.
 * g = grad_scale * grad (1 / world after the all-reduce sum), clipped to max_norm by its global 2-norm (max_norm <= 0: no clip),
 * then Adam step number `step` (1-based; bias corrections evaluated in double on the host).  ONE launch, fixed summation order:
 * the same inputs give the same bits on every rank.  norm_out (device, may be NULL) receives the unclipped norm of g. */
int irrl_clip_adam(int n, float *theta, const float *grad, float *m, float *v, float grad_scale, float max_norm, float lr, float beta1, float beta2,
                   float eps, long long step, float *norm_out, void *hip_stream);

/* out[map[m][c]] = (add ? add[m][c] : 0) + sum over r of part[m][r][c]  for the nmat matrices part [nmat, rows, cols] of per-workgroup
 * partial sums (fixed order); map [nmat, cols] int32 (device), entries < 0 skip the column.  Used to drop the MlpPolicy gradient kernels'
 * partial rows straight into the flat gradient buffer in parameter layout. */
int irrl_sum_rows_scatter(const float *part, int nmat, int rows, int cols, const int *map, const float *add, float *out, void *hip_stream);

/* out[i] = E(i), i < n: a keyed random permutation of 0 .. n-1 (int64, device) in ONE launch and without a sort -- the shuffled sample order of
 * an optimisation epoch (ppo2.py:364-380).  E = 4-round Feistel network on the bits of n - 1 with cycle walking; depends on (n, seed, counter)
 * only; `ppo2.feistel_permutation` is the numpy twin. */
int irrl_random_permutation(long long n, unsigned seed, unsigned counter, long long *out, void *hip_stream);

/* synthetic action stream of the benchmark (a = clip(sigma N(0,1), -1, 1) from Philox(seed, stream = env,
 * counter = step)): fills out[n_steps][n_envs][12] (device) for envs env0 .. and steps step0 ..; values depend only on
 * (seed, global env id, step), not on the shape of the request.  tests/ hold the numpy twin. */
int irrl_bench_actions(unsigned seed, int env0, int n_envs, long long step0, int n_steps, float sigma, float *out, void *hip_stream);

/* PMC calibration helper: copies n floats with one dword per lane (the env kernels' access width) so that
 * FETCH_SIZE / WRITE_SIZE can be calibrated on a known byte count (MI355X_MICROARCH.md, HBM section). */
int irrl_calib_copy_dword(const float *src, float *dst, size_t n, void *hip_stream);

/* ---- persistent LSTM sequence kernels for the PPO2 update (stable-baselines lstm of CustomLSTMPolicy,
 * run_bp_v5.py:143-176; the train graph unrolls all n_steps, ppo2.py:132-134).  Device pointers, f32.
 * Gate columns are in [unit][gate] order (gate = i,f,o,g): zx/gates/dz [T,N,hid,4], cseq/hseq/dh_in [T,N,hid],
 * masks [T,N] (1.0 = done before step t), state0/state_out [N,2*hid] = [c|h], wh_p [hid][hid][4].
 * hid in {32,48,64}, N % 16 == 0.  Returns 0, or 1 for an unsupported shape, 2 for a launch error. */
int irrl_lstm_seq_forward(int hid, int T, int N, const float *zx, const float *wh_p, const float *masks, const float *state0,
                          float *gates, float *cseq, float *hseq, float *state_out, void *hip_stream);
/* the same forward pass with the input projection fused in (no zx tensor): x [T,N,n_in] is the layer input,
 * wx_p [n_in][hid][4], b_p [hid][4]; n_in <= 48 */
int irrl_lstm_seq_forward_x(int hid, int T, int N, int n_in, const float *x, const float *wx_p, const float *b_p, const float *wh_p,
                            const float *masks, const float *state0, float *gates, float *cseq, float *hseq, float *state_out,
                            void *hip_stream);
int irrl_lstm_seq_backward(int hid, int T, int N, const float *gates, const float *cseq, const float *masks, const float *state0,
                           const float *dh_in, const float *wh_p, float *dz, void *hip_stream);

/* out[c] = sum over rows of part[rows, cols] in one fixed order (the per-workgroup partial sums the gradient kernels leave);
 * unit_gate_hid > 0 also undoes the [unit][gate] column permutation inside each group of 4 * hid columns (out column g * hid + u
 * <- partial column 4 u + g).  Returns 0, 1 = bad shape, 2 = launch error. */
int irrl_sum_rows(const float *part, int rows, int cols, int unit_gate_hid, float *out, void *hip_stream);

/* backward pass with everything that consumes dz fused in (no dz tensor, no separate weight-gradient GEMMs):
 * hseq / x are the forward outputs / inputs; dx [T,N,n_in] or NULL; dwx_part [N/16, n_in, 4 hid], dwh_part [N/16, hid,
 * 4 hid], db_part [N/16 * 4, 4 hid] receive per-workgroup partial sums (permuted gate columns) that the caller adds up
 * over their first axis.  n_in <= 48. */
int irrl_lstm_seq_backward_x(int hid, int T, int N, int n_in, const float *gates, const float *cseq, const float *hseq, const float *x,
                             const float *masks, const float *state0, const float *dh_in, const float *wh_p, const float *wx_p,
                             float *dx, float *dwx_part, float *dwh_part, float *db_part, void *hip_stream);

/* the same two sequence kernels on the bf16 matrix cores with COMPENSATED OPERAND SPLITS and f32 accumulation (csrc/lstm_bf16.hpp; hid 48,
 * n_in <= 48): every operand is split into nsplit bf16 planes (2: ~2^-16 relative product error, 3: ~2^-24, the f32 level) and a product is the
 * sum of the plane products above that weight (3 resp. 6 MFMAs); v_mfma_f32_16x16x32_bf16 covers 32 units of K in half the time the exact-f32
 * v_mfma_f32_16x16x4_f32 needs for 4.  Tensors, layouts and return codes as irrl_lstm_seq_forward_x / irrl_lstm_seq_backward_x. */
/* (forward: gates == NULL and cseq == NULL selects the INFERENCE form -- only hseq and state_out are written: the critic pass behind an actor-only rollout;
 * gates == NULL with cseq given: c and h are kept, the gates are not -- the forward half of a backward pass that RECOMPUTES them.
 * backward: gates == NULL (nsplit 2 only; b_p = the layer's permuted bias, otherwise unused and may be NULL) runs the kernel that forms
 * z_t = b + [h_{t-1} keep_t | x_t] [wh ; wx] itself from the h / x tiles it stages for the weight gradients anyway -- the forward kernel's products,
 * plane for plane and in its order, so every output equals the gate-loading kernel's bit for bit; round 6) */
int irrl_lstm_seq_forward_bf16(int nsplit, int hid, int T, int N, int n_in, const float *x, const float *wx_p, const float *b_p, const float *wh_p,
                               const float *masks, const float *state0, float *gates, float *cseq, float *hseq, float *state_out, void *hip_stream);
int irrl_lstm_seq_backward_bf16(int nsplit, int hid, int T, int N, int n_in, const float *gates, const float *cseq, const float *hseq, const float *x,
                                const float *masks, const float *state0, const float *dh_in, const float *wh_p, const float *wx_p, const float *b_p,
                                float *dx, float *dwx_part, float *dwh_part, float *db_part, void *hip_stream);

/* ---- one ROLLOUT step of CustomLSTMPolicy in a single launch (run_bp_v5.py:178-185 `step`; the runner's clip and
 * buffer rows, ppo2.py:521-535).  Two stacks (actor, critic) of two LSTM layers of `hid` units, heads pi [hid,act],
 * vf [hid,1], logstd [act].  lstm_w is a HOST array of 12 device pointers: for layer in (pi0, pi1, v0, v1):
 * wx_p [n_in][hid][4], wh_p [hid][hid][4], b_p [hid][4] (gate columns in [unit][gate] order).  states [N, 8 hid] =
 * pi0 [c|h], pi1 [c|h], v0 [c|h], v1 [c|h]; states_out may alias states_in.
 * Sampling noise: `noise` [N,act] ~ N(0,1) if not NULL; else rng_on = 1 draws it in the kernel from the engine's
 * counter RNG (Philox4x32-10, key (rng_seed,'IRR1'), counter (env, step >> 32, step, 0x50 + a/4), Box-Muller on the
 * pairs (u0,u1), (u2,u3)) with step = rng_step + *rng_base (rng_base: device int64 scalar or NULL); else
 * deterministic (action = mean).
 * Outputs action (unclipped sample), clipped (to [-1,1]), value [N], neglogp [N].  With row >= 0 also row `row` of
 * mb_obs [T,N,ob], mb_actions [T,N,act], mb_values / mb_neglogp [T,N], mb_dones [T,N] u8, and, if mb_rewards and
 * prev_reward [N] are given and row > 0, row-1 of mb_rewards (the reward of the previous env step).
 * Any N (workgroups of 16 envs, the last one partially filled), hid in {32,48,64}, 16 act + 16 <= 8 hid. */
int irrl_lstm_policy_step(int hid, int ob_dim, int act_dim, int N, const float *obs, const uint8_t *dones, const float *states_in,
                          float *states_out, const float *const *lstm_w, const float *pi_w, const float *pi_b, const float *vf_w,
                          const float *vf_b, const float *logstd, const float *noise, int rng_on, unsigned rng_seed, long long rng_step,
                          const long long *rng_base, int env_id_offset, float *action, float *clipped, float *value, float *neglogp, long long row, float *mb_obs,
                          float *mb_actions, float *mb_values, float *mb_neglogp, uint8_t *mb_dones, float *mb_rewards,
                          const float *prev_reward, void *hip_stream);

/* (env_id_offset in the three policy entry points: global id of env 0 -- the in-kernel sampling noise of env e is the counter RNG's
 * stream e + env_id_offset, so an N-GPU job whose ranks pass rank * N draws exactly the noise of the one big pool.)
 * `steps` consecutive rollout steps (policy step t, then env.step on its clipped action) launched back to back by ONE call on
 * `hip_stream`: step k runs irrl_lstm_policy_step with rng_step + k, row + k and noise + k N act (if noise is given: a
 * [steps, N, act] table), states updated in place (states_out may equal states_in), and then the env step of pool `env`
 * (N = its num_envs) that writes obs / dones IN PLACE (the arrays the next policy step reads), the reward to `env_reward` [N]
 * (= prev_reward of the next policy step) and the extras to `env_extra` [N,6].  What ppo2.Runner used to record as a hipGraph of
 * 2 x steps kernel nodes (same speed, no capture).  fuse != 0: env.step k and the policy step k + 1 run as ONE launch (a workgroup =
 * the four env waves of 16 robots = one MFMA M-tile; 16-lane layout, hid 48, no Crutial; otherwise ignored) -- bit-identical
 * results, measured slower than the two-launch sequence on MI355X.  fuse == 2: the whole rollout as ONE persistent launch (a workgroup
 * loops over all `steps` for its 16 robots: no grid-wide boundary between steps; same conditions, otherwise the two-launch sequence) --
 * bit-identical results again.  fuse == 3 (round 5): that persistent launch with the CRITIC OFF THE PER-STEP PATH -- V(s_t) depends on the observation
 * history only and nothing in the rollout needs it before GAE, so the per-step part runs the actor stack alone (all of its operands resident in LDS) and
 * writes everything EXCEPT `value` / `mb_values` and the critic's half of `states`, which the caller obtains for the whole rollout afterwards with the
 * sequence kernels over the recorded observations (ppo2.Runner does); actor-side buffers bit-identical to the other modes; an error where the persistent
 * kernel is not instantiated.
 * WHICH POOLS GET THE SINGLE LAUNCH (fuse 1 / 2 / 3): 16 lanes per robot, hid 48, kernel variant "md", "shipped" or "shipped_flat" -- the published
 * contact rule without the meteorite, with the shipped solver settings or any others (a config without the Contact* keys, ContactSolver 1, another
 * sweep cap, a control step of other than eight substeps).  Crutial pools, ContactSolver 0 / 2 and 4-lane pools run two launches per step. */
int irrl_lstm_rollout(irrl_env *env, int steps, int hid, int ob_dim, int act_dim, float *obs, uint8_t *dones, const float *states_in,
                      float *states_out, const float *const *lstm_w, const float *pi_w, const float *pi_b, const float *vf_w,
                      const float *vf_b, const float *logstd, const float *noise, int rng_on, unsigned rng_seed, long long rng_step,
                      const long long *rng_base, int env_id_offset, float *action, float *clipped, float *value, float *neglogp, long long row, float *mb_obs,
                      float *mb_actions, float *mb_values, float *mb_neglogp, uint8_t *mb_dones, float *mb_rewards,
                      float *env_reward, float *env_extra, int fuse, void *hip_stream);

/* Which `fuse` modes of irrl_lstm_rollout exist for THIS pool and a network of `hid` units per LSTM layer: 1 = the mode runs as described above,
 * 0 = it does not (fuse 1 / 2 then run as two launches per step inside the call; fuse 3 is refused with an error, because its caller has to
 * evaluate the critic itself and must know beforehand), -1 = bad handle.  Callers branch on this, not on the text of irrl_last_error(). */
int irrl_lstm_rollout_supports(irrl_env *env, int hid, int fuse);

/* the same single-launch rollout step for MlpPolicy (flex_gym/archi/policies.py:430-446: separate pi / vf nets of two tanh
 * layers of `hid` = 64 units).  mlp_w: HOST array of 8 device pointers pi_w1 [ob][hid], pi_b1, pi_w2 [hid][hid], pi_b2,
 * vf_w1, vf_b1, vf_w2, vf_b2; heads, sampling, outputs and rollout rows as above; act <= 15. */
int irrl_mlp_policy_step(int hid, int ob_dim, int act_dim, int N, const float *obs, const uint8_t *dones, const float *const *mlp_w,
                         const float *pi_w, const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, const float *noise,
                         int rng_on, unsigned rng_seed, long long rng_step, const long long *rng_base, int env_id_offset, float *action, float *clipped,
                         float *value, float *neglogp, long long row, float *mb_obs, float *mb_actions, float *mb_values, float *mb_neglogp,
                         uint8_t *mb_dones, float *mb_rewards, const float *prev_reward, void *hip_stream);

/* `steps` consecutive rollout steps of MlpPolicy (policy step t, then env.step on its clipped action) from ONE call -- the MlpPolicy twin of
 * irrl_lstm_rollout (no recurrent state; mlp_w as in irrl_mlp_policy_step; ob 35, act 12, hid 64).  fuse == 2 and a pool the combined
 * kernel exists for (16 lanes per robot, kernel variant "md", "shipped" or "shipped_flat": Crutial off, published contact rule, any solver
 * settings and substep count): the whole rollout as ONE persistent launch -- a workgroup
 * keeps its 16 robots and the policy's weights (in LDS) for all `steps`, no grid-wide boundary between steps; otherwise 2 x steps launches
 * back to back.  Bit-identical buffers either way (what ppo2.Runner records as a hipGraph of 2 x steps nodes otherwise). */
int irrl_mlp_rollout(irrl_env *env, int steps, int hid, int ob_dim, int act_dim, float *obs, uint8_t *dones, const float *const *mlp_w, const float *pi_w,
                     const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, const float *noise, int rng_on, unsigned rng_seed,
                     long long rng_step, const long long *rng_base, int env_id_offset, float *action, float *clipped, float *value, float *neglogp,
                     long long row, float *mb_obs, float *mb_actions, float *mb_values, float *mb_neglogp, uint8_t *mb_dones, float *mb_rewards,
                     float *env_reward, float *env_extra, int fuse, void *hip_stream);

/* which `fuse` modes of irrl_mlp_rollout exist for THIS pool and a network of `hid` units: 1 = the mode runs as described (fuse 0 always; fuse 2 where
 * the persistent kernel exists), 0 = it does not (fuse 2 then runs as 2 x steps launches inside the call; hid != 64 is refused by irrl_mlp_rollout),
 * -1 = bad handle.  The twin of irrl_lstm_rollout_supports. */
int irrl_mlp_rollout_supports(irrl_env *env, int hid, int fuse);

/* ---- DEVICE-RESIDENT POLICY EVALUATION (run_bp_v5.py:353-470, the reference's robustness study: friction, observation delay, rate / action
 * low-passes, command ramp).  `steps` control steps of the closed loop  conditioning -> CustomLSTMPolicy (deterministic) -> action filter ->
 * env.step -> record  issued by ONE call as plain launches back to back on `hip_stream` (five per step; kernels csrc/eval_rollout.hpp, the policy
 * step and the env step are the existing ones, so every pool kind and kernel variant works).  Nothing is captured, nothing synchronises, and the
 * call keeps no state: a second call with step0 + steps continues exactly where the first stopped.  The persistent single-launch form of the same
 * loop is irrl_lstm_eval_rollout_persistent below.
 *
 * Control step t = step0 + k, per env e:
 *    1. cmd = (1 - a_cmd) cmd + a_cmd cmd_target            2. ring[t % D] = obs              3. o = ring[(t - delay_e) mod D]
 *    4. o[17:29], o[32:35] = (1 - a_vel) vel_his + a_vel o   5. vel_his = o (whole vector)     6. o[0:3] = (cmd - cmd_mean) / cmd_std
 *    7. the actor on o (irrl_lstm_policy_step without noise: it resets the LSTM state of an env whose `done` is set)
 *    8. a = clipped mean (clip != 0) or the mean             9. a = (1 - a_act) act_his + a_act a   10. act_his = a
 *   11. env.step(a) -> obs, done                            12. recorders, statistics          13. cmd = 0 where done
 * A coefficient a_* = 2 pi dt f / (2 pi dt f + 1) of EXACTLY 1.0f switches that filter off (values pass bit for bit).  The ring and the filter
 * histories are not cleared by an in-episode `done` (the script does not clear them either).
 *
 * Evaluator state, caller-owned device memory (N = num_envs of `env`, D = depth >= 1): ring [D, N, 35], cmd [N, 3], vel_his [N, 35], act_his [N, 12],
 * lstm_state [N, 8 hid], done [N] u8, obs [N, 35] (raw observation: in = the last env output / the reset observation, out = the last step's),
 * work [N, IRRL_EVAL_WORK_DIM] f32 scratch.  A fresh evaluation: obs = irrl_env_reset's, every plane of ring = obs, everything else zero.
 * Per-env parameters (device): delay [N] int32 in 0 .. D-1 (the caller validates; values outside are clamped), cmd_target [N, 3].
 * Scalars: a_cmd, a_vel, a_act in (0, 1]; cmd_mean / cmd_std: HOST arrays of 3 floats (scaling of obs[0:3], Environment.hpp:371-393).
 * lstm_w (HOST array of 12 device pointers), the heads and hid / ob_dim / act_dim as irrl_lstm_policy_step; hid in {32, 48, 64}, ob 35, act 12.
 * Recorders (device, each may be NULL = off), row k = step k OF THIS CALL: rec_obs_cond [steps, N, 35] (what the actor saw), rec_act_clipped /
 * rec_act_applied [steps, N, 12] (before / after the action filter), rec_body [steps, N, 13] = base x y z, quaternion wxyz, world linear and
 * angular velocity after the env step (the layout of the reference's body-center logs), rec_torque [steps, N, 12], rec_obs_raw [steps, N, 35],
 * rec_reward [steps, N], rec_done [steps, N] u8.
 * stats (device f64 [IRRL_EVAL_STAT_COUNT, N], may be NULL): per-env accumulators over the recorded body frames, ADDED to by every step (zero them
 * to start a window; one thread owns one env's column, no atomics; body frame, roll = atan2, pitch = asin evaluated in f64).
 * Errors (non-zero, irrl_last_error() set, checked before any HIP call): NULL handle, depth < 1, hid outside {32, 48, 64}, ob_dim != 35,
 * act_dim != 12, a NULL state / parameter / weight pointer, a coefficient outside (0, 1]. */
#define IRRL_EVAL_WORK_DIM 80 /* obs_cond 35 | action 12 | clipped 12 | applied 12 | value | neglogp | reward | extra 6 */
enum {
  IRRL_EVAL_STAT_N = 0,     /* frames accumulated */
  IRRL_EVAL_STAT_VX, IRRL_EVAL_STAT_VX2,       /* sum, sum of squares: body-frame v_x */
  IRRL_EVAL_STAT_Z, IRRL_EVAL_STAT_Z2,         /* base height */
  IRRL_EVAL_STAT_ROLL, IRRL_EVAL_STAT_ROLL2,
  IRRL_EVAL_STAT_PITCH, IRRL_EVAL_STAT_PITCH2,
  IRRL_EVAL_STAT_WX, IRRL_EVAL_STAT_WX2,       /* body-frame roll rate */
  IRRL_EVAL_STAT_WY, IRRL_EVAL_STAT_WY2,       /* body-frame pitch rate */
  IRRL_EVAL_STAT_VZ, IRRL_EVAL_STAT_VZ2,       /* world v_z */
  IRRL_EVAL_STAT_VY,        /* sum of body-frame v_y */
  IRRL_EVAL_STAT_WZ,        /* sum of world omega_z */
  IRRL_EVAL_STAT_FALLS,     /* number of steps that ended in `done` */
  IRRL_EVAL_STAT_COUNT
};
int irrl_lstm_eval_rollout(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w, const float *pi_w,
                           const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring, float *cmd, float *vel_his,
                           float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay, const float *cmd_target, float a_cmd,
                           float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip, float *rec_obs_cond, float *rec_act_clipped,
                           float *rec_act_applied, float *rec_body, float *rec_torque, float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats,
                           void *hip_stream);

/* THE SAME LOOP AS ONE PERSISTENT LAUNCH (kernel csrc/env_eval_kernels.hpp): a wave keeps its four robots -- lane context and LSTM cell state in
 * registers, h, the filter histories, the command and the statistics in LDS -- for all `steps` control steps; no grid-wide boundary between steps.
 * Same argument list, same order, same per-element arithmetic (csrc/eval_elements.hpp): every recorder, stats, ring, cmd, vel_his, act_his, done, obs,
 * the pool, the ACTOR's half of lstm_state ([:, 0 : 4 hid]) and the work columns obs_cond | action | clipped | applied | reward | extra are
 * BIT-IDENTICAL to irrl_lstm_eval_rollout's.  The critic is not run: the critic's half of lstm_state ([:, 4 hid : 8 hid]) and the `value` column of
 * the work array are left untouched.  The actor never reads them, so calls of either form may follow each other on the same buffers.
 * irrl_lstm_eval_rollout_supports: 1 = the kernel exists for this pool and a network of `hid` units -- exactly where
 * irrl_lstm_rollout_supports(env, hid, 3) is 1: 16 lanes per robot, hid 48, kernel variant shipped_flat / shipped / md --, 0 = it does not,
 * -1 = NULL handle (irrl_last_error() set).
 * irrl_lstm_eval_rollout_persistent makes the refusals of irrl_lstm_eval_rollout before any HIP call, with its own name in the texts, and refuses
 * a pool or `hid` without the kernel with a text that names the failed condition: there is NO fallback inside the call.  steps == 0 returns 0 and
 * launches nothing. */
int irrl_lstm_eval_rollout_supports(irrl_env *env, int hid);
int irrl_lstm_eval_rollout_persistent(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w,
                                      const float *pi_w, const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring,
                                      float *cmd, float *vel_his, float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay,
                                      const float *cmd_target, float a_cmd, float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip,
                                      float *rec_obs_cond, float *rec_act_clipped, float *rec_act_applied, float *rec_body, float *rec_torque,
                                      float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats, void *hip_stream);

/* THE EVALUATION LOOP WITH A SCENARIO: a command schedule, a heading hold and statistics per time segment, the three ingredients of the reference's
 * evaluation loop that need the loop's own step counter or the robot's state at every control step (run_bp_v5.py:383-388 `--step`, :308-315 and
 * :400-406 `--dir_fd`).  Semantics in ONE text, csrc/eval_elements.hpp.  With tau = max(t - t0, 0) for control step t (t = step0 + k, the
 * evaluator's global counter) and env e:
 *   command schedule   cmd_target of step 1 above becomes cmd_table[min(tau / cmd_every, cmd_rows - 1), e, 0:3] (device f32 [cmd_rows, N, 3]); the
 *                      last row holds once the table runs out; cmd_every = 1: one row per step.  Filters, delay line, scaling unchanged.
 *   heading hold       on for env e where heading_kp[e] != 0 || heading_ki[e] != 0 (device f32 [N] each; all three NULL = off for everyone).  With
 *                      q the base quaternion as the pool holds it at conditioning time (after step t - 1, or after the reset; not delayed), in f32:
 *                      yaw = atan2f(2 (w z + x y), 1 - 2 (y y + z z)); err = heading_ref[e] - yaw wrapped into [-pi, pi);
 *                      I_e = clamp(I_e + err heading_dt, -heading_windup, +heading_windup); out = kp_e err + ki_e I_e; the actor's element 2 is
 *                      (out - cmd_mean[2]) / cmd_std[2] in place of the scaled low-passed command (cmd[e, 2] keeps evolving unseen).  I_e lives
 *                      in heading_int (device f32 [N], caller-owned state like cmd) and is zeroed where the env step ends in `done`.  The common
 *                      positional PID with Kd = 0 and an integrator clamp (the reference's utils/PID.py is not in its tree).
 *   statistics buckets the frame of step t is added to stats[min(tau / stat_every, stat_buckets - 1)]: stats is [stat_buckets,
 *                      IRRL_EVAL_STAT_COUNT, N]; stat_buckets = 1 is the plain buffer.
 * scenario == NULL is exactly irrl_lstm_eval_rollout[_persistent], which are calls of these with NULL.  Both forms leave bit-identical buffers
 * (heading_int included); the persistent one exists exactly where irrl_lstm_eval_rollout_supports says so, with no fallback inside the call.
 * Refused before any HIP call, with the entry point's name in the text: cmd_rows / cmd_every / stat_buckets / stat_every < 1, a NULL cmd_table,
 * a partly NULL heading set, heading on without heading_int, heading_windup < 0, heading_dt <= 0 (the last two where the heading set is given). */
typedef struct irrl_eval_scenario {
  long long t0;
  int cmd_rows, cmd_every;
  const float *cmd_table;
  int stat_buckets, stat_every;
  const float *heading_ref, *heading_kp, *heading_ki;
  float *heading_int;
  float heading_windup, heading_dt;
} irrl_eval_scenario;
int irrl_lstm_eval_scenario(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w, const float *pi_w,
                            const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring, float *cmd, float *vel_his,
                            float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay, const float *cmd_target, float a_cmd,
                            float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip, float *rec_obs_cond, float *rec_act_clipped,
                            float *rec_act_applied, float *rec_body, float *rec_torque, float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats,
                            const irrl_eval_scenario *scenario, void *hip_stream);
int irrl_lstm_eval_scenario_persistent(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w,
                                       const float *pi_w, const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring,
                                       float *cmd, float *vel_his, float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay,
                                       const float *cmd_target, float a_cmd, float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip,
                                       float *rec_obs_cond, float *rec_act_clipped, float *rec_act_applied, float *rec_body, float *rec_torque,
                                       float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats, const irrl_eval_scenario *scenario,
                                       void *hip_stream);

/* THE EVALUATION LOOP WITH A KICK TABLE: caller-specified displacements of the robots' base state at chosen control steps, the ingredient of the
 * reference's perturbation exploration (Exp_Raw_Data/Param-*.txt: NoE explorations of FoE steps from a base state displaced by z_noise, roll_noise,
 * pitch_noise, *_dot_noise).  Semantics in ONE text, csrc/eval_elements.hpp.  A kick row is IRRL_EVAL_KICK_DIM = 11 floats per env,
 *   dz | dq_w dq_x dq_y dq_z | dv_x dv_y dv_z | dw_x dw_y dw_z
 * body-frame: with q the base quaternion and R(q) its rotation matrix BEFORE the kick, all in f32,
 *   z += dz;   v_w += R(q) dv  (gv[0:3]);   w_w += R(q) dw  (gv[3:6]);   q = (q (x) dq) / |q (x) dq|.
 * x, y, the joints and every other array of the pool are untouched: what a set_state of those ten words would do.  A row whose four dq words are
 * all zero is "no kick for this env": the env is untouched bit for bit whatever the other seven words are.  The identity kick is dq = (1, 0, 0, 0)
 * with everything else zero; it is a real kick (it renormalises).  dq from roll / pitch / yaw increments is host work; the device does no
 * trigonometry.
 * Schedule: with t0 the scenario's where one is given and 0 otherwise, row r of kick_table (device f32 [kick_rows, N, 11]) fires at the control
 * step t with t >= t0 + kick_first and t - t0 - kick_first = r kick_every, 0 <= r < kick_rows.  The kick hits at the start of env step t: after
 * the actor and the action filter of step t, on the state that step t - 1 (or the reset) left; the actor first sees it in the observation of
 * step t + 1 (plus the env's delay); the heading hold of step t reads the pre-kick quaternion.
 * kicks == NULL is exactly irrl_lstm_eval_scenario[_persistent], which are calls of these with NULL.  Both forms leave bit-identical buffers; the
 * five-launch form issues one extra launch (the kernel of irrl_env_perturb_base) at a step whose row fires and none elsewhere; the persistent one
 * exists exactly where irrl_lstm_eval_rollout_supports says so, with no fallback inside the call.
 * Refused before any HIP call, with the entry point's name in the text: kick_rows < 1, kick_every < 1, kick_first < 0, a NULL kick_table. */
#define IRRL_EVAL_KICK_DIM 11
typedef struct irrl_eval_kicks {
  int kick_rows;
  long long kick_first;
  int kick_every;
  const float *kick_table;
} irrl_eval_kicks;
int irrl_lstm_eval_perturbed(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w, const float *pi_w,
                             const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring, float *cmd, float *vel_his,
                             float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay, const float *cmd_target, float a_cmd,
                             float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip, float *rec_obs_cond, float *rec_act_clipped,
                             float *rec_act_applied, float *rec_body, float *rec_torque, float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats,
                             const irrl_eval_scenario *scenario, const irrl_eval_kicks *kicks, void *hip_stream);
int irrl_lstm_eval_perturbed_persistent(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w,
                                        const float *pi_w, const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring,
                                        float *cmd, float *vel_his, float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay,
                                        const float *cmd_target, float a_cmd, float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip,
                                        float *rec_obs_cond, float *rec_act_clipped, float *rec_act_applied, float *rec_body, float *rec_torque,
                                        float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats, const irrl_eval_scenario *scenario,
                                        const irrl_eval_kicks *kicks, void *hip_stream);
/* One kick row per env applied to the pool NOW, stream-ordered on the pool's stream (the same device function; the kernel the five-launch form
 * launches at a kick step): rows is device f32 [N, 11] (irrl_env_perturb_base) or host f32 [N, 11] (irrl_env_perturb_base_host, which waits for
 * the stream).  Any pool kind and lane layout: only the pool's gc[2:7] and gv[0:6] are written.  A NULL handle or NULL rows is refused before
 * any HIP call. */
int irrl_env_perturb_base(irrl_env *env, const float *rows);
int irrl_env_perturb_base_host(irrl_env *env, const float *rows);

/* THE EVALUATION LOOP WITH GAIT MEASUREMENTS: joint mechanical power, torque and ground-force sums and the footfall pattern at control-step rate,
 * the quantities of the reference's own analysis of its evaluation runs (Data_Visualization_Code/Figure2.py:62-63 power = sum_j qd_j tau_j per
 * control step, :198-222 TCoT = P / (m g v) per command level, :36 and :97-116 the gait diagrams out of the contact flags; run_bp_v5.py:446-457
 * logs the same words every step).  Semantics in ONE text, csrc/eval_elements.hpp irrl_eval_gait_epilogue.  After the env step of control step t,
 * with the words the pool holds then -- tq = torque [N, 12], qd = gv[:, 6:18], in_contact [N, 4] and lam_w [N, 4, 3] -- an env whose step did NOT
 * end in `done` adds one frame to its column of
 *   gait (device f64 [stat_buckets, IRRL_EVAL_GAIT_COUNT, N]; bucket = the bucket of `stats`, one without a scenario),
 * every f32 word widened to f64 first, sums added in index order (j = 0 .. 11, leg = 0 .. 3); rows IRRL_EVAL_GAIT_* below.  A step that ends in
 * `done` adds nothing (its words are the reset state, not a sample of the gait).  Every step, `done` or not, then sets prev_contact[e, leg] =
 * (in_contact != 0); prev_contact is caller-owned evaluator state, device u8 [N, 4], zero for a fresh evaluation.  The PEAK rows are running
 * maxima, not sums: buckets and envs combine with max.
 * WHAT lam_w IS: the world-frame contact IMPULSE (N s) of the LAST physics substep of the control step, zero for a leg that substep did not
 * have in the contact list -- the contact solve overwrites it every substep; it is not the control step's sum.  The env's contact reward scales
 * its norm by 1 / control_dt and so do the rows here: GRFZ and PEAK_GRF are in the reward's unit, lam_w / control_dt, which is the mean force
 * of the last substep times simulation_dt / control_dt.  Divide by that ratio on the host for newtons.
 * rec_gait (device f32 [steps, N, IRRL_EVAL_GAIT_REC_DIM], may be NULL = off), row k = step k of this call, `done` steps included:
 *   tq 12 | qd 12 | in_contact 4 (0.0 / 1.0) | lam_w_z * (1 / control_dt) 4 (the f32 product)
 * gait == NULL (the struct pointer) is exactly irrl_lstm_eval_perturbed[_persistent], which are calls of these with NULL; IRRL_EVAL_STAT_COUNT and
 * the layout of `stats` are unchanged.  Both forms leave bit-identical buffers (gait, prev_contact, rec_gait included); the persistent one exists
 * exactly where irrl_lstm_eval_rollout_supports says so, with no fallback inside the call.  Every pool kind and lane layout for the other.
 * Refused before any HIP call, with the entry point's name in the text: a struct with `gait` set and prev_contact NULL; a struct whose three
 * pointers are all NULL.  rec_gait alone (prev_contact NULL or not) is the recorder only; prev_contact alone keeps the flags up to date through
 * steps that are not measured (a warm-up), so that the first measured step sees its predecessor's. */
enum {
  IRRL_EVAL_GAIT_N = 0,            /* frames added (steps that did not end in `done`) */
  IRRL_EVAL_GAIT_P, IRRL_EVAL_GAIT_P2,        /* p = sum_j tq_j qd_j (W): sum, sum of squares */
  IRRL_EVAL_GAIT_PPOS, IRRL_EVAL_GAIT_PNEG,   /* sum_j max(tq_j qd_j, 0), sum_j min(tq_j qd_j, 0) */
  IRRL_EVAL_GAIT_TAU2,             /* sum of tq_j^2 over the 8 abad / hip joints */
  IRRL_EVAL_GAIT_TAU2_KNEE,        /* sum of tq_j^2 over the 4 knee joints (j % 3 == 2) */
  IRRL_EVAL_GAIT_PEAK_TAU, IRRL_EVAL_GAIT_PEAK_QD,   /* running max of |tq_j|, |qd_j| */
  IRRL_EVAL_GAIT_STANCE0, IRRL_EVAL_GAIT_STANCE1, IRRL_EVAL_GAIT_STANCE2, IRRL_EVAL_GAIT_STANCE3,           /* frames with the leg in contact */
  IRRL_EVAL_GAIT_TOUCHDOWN0, IRRL_EVAL_GAIT_TOUCHDOWN1, IRRL_EVAL_GAIT_TOUCHDOWN2, IRRL_EVAL_GAIT_TOUCHDOWN3,   /* prev_contact == 0 && in_contact != 0 */
  IRRL_EVAL_GAIT_FLIGHT,           /* frames with no leg in contact */
  IRRL_EVAL_GAIT_GRFZ,             /* sum over legs in contact of (double)(lam_w_z * (1 / control_dt)) */
  IRRL_EVAL_GAIT_PEAK_GRF,         /* running max over legs in contact of |lam_w| * (1 / control_dt), the norm in f64 */
  IRRL_EVAL_GAIT_COUNT
};
#define IRRL_EVAL_GAIT_REC_DIM 32
typedef struct irrl_eval_gait {
  double *gait;
  uint8_t *prev_contact;
  float *rec_gait;
} irrl_eval_gait;
int irrl_lstm_eval_measured(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w, const float *pi_w,
                            const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring, float *cmd, float *vel_his,
                            float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay, const float *cmd_target, float a_cmd,
                            float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip, float *rec_obs_cond, float *rec_act_clipped,
                            float *rec_act_applied, float *rec_body, float *rec_torque, float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats,
                            const irrl_eval_scenario *scenario, const irrl_eval_kicks *kicks, const irrl_eval_gait *gait, void *hip_stream);
int irrl_lstm_eval_measured_persistent(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w,
                                       const float *pi_w, const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring,
                                       float *cmd, float *vel_his, float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay,
                                       const float *cmd_target, float a_cmd, float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip,
                                       float *rec_obs_cond, float *rec_act_clipped, float *rec_act_applied, float *rec_body, float *rec_torque,
                                       float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats, const irrl_eval_scenario *scenario,
                                       const irrl_eval_kicks *kicks, const irrl_eval_gait *gait, void *hip_stream);

/* THE EVALUATION LOOP WITH MlpPolicy AS THE ACTOR (policies.py MlpPolicy: separate pi / vf nets of two tanh layers of 64 units): the loop above,
 * steps 1-13, with irrl_mlp_policy_step in step 7's place.  ONE widest pair of entry points: the argument list is irrl_lstm_eval_measured's with
 * mlp_w (HOST array of 8 device pointers, as irrl_mlp_policy_step takes it) where lstm_w is, and WITHOUT lstm_state -- the policy has no recurrent
 * state; `done` still drives cmd = 0 (step 13) and the heading integrator.  hid must be 64, ob_dim 35, act_dim 12.  scenario, kicks and gait may
 * each be NULL = none, exactly as the irrl_lstm_eval_* entry points treat them; evaluator state, parameters, recorders, stats and the three
 * structs are theirs, unchanged.  The policy runs deterministically: no noise, rng off, no rollout rows.
 *   irrl_mlp_eval_measured              `steps` control steps as plain launches back to back (five per step, a sixth at a kick step); every pool
 *                                       kind, kernel variant and lane layout.
 *   irrl_mlp_eval_measured_persistent   the same call as ONE persistent launch (kernel csrc/env_eval_mlp_kernels.hpp): a wave keeps its four robots
 *                                       -- lane context in registers; weights, filter histories, command, statistics and gait accumulators in LDS
 *                                       -- for all `steps` control steps.
 * WHAT BOTH FORMS WRITE, BIT-IDENTICALLY: every recorder (rec_gait included), stats, gait, prev_contact, heading_int, ring, cmd, vel_his, act_his,
 * done, obs, the pool, and EVERY column of the work array the per-step form writes: obs_cond | action | clipped | applied | value | neglogp | reward |
 * extra.  The persistent kernel runs both networks (the per-wave body of irrl_mlp_policy_step's kernel), so -- unlike the LSTM pair -- `value` and
 * `neglogp` are written by both forms; no column stays untouched.  Calls of either form may follow each other on the same buffers.
 * irrl_mlp_eval_rollout_supports: 1 = the persistent kernel exists for this pool and a network of `hid` units -- exactly where
 * irrl_mlp_rollout_supports(env, 64, 2) is 1: 16 lanes per robot, kernel variant shipped_flat / shipped / md, hid 64 --, 0 = it does not,
 * -1 = NULL handle (irrl_last_error() set).
 * Errors (non-zero, irrl_last_error() set with the entry point's own name, checked before any HIP call): the refusals of irrl_lstm_eval_measured
 * with "hid is 64" for any other hid and an 8-entry weight table; irrl_mlp_eval_measured_persistent also refuses a pool without the kernel with a
 * text that names the failed condition: there is NO fallback inside the call.  steps == 0 returns 0 and launches nothing. */
int irrl_mlp_eval_rollout_supports(irrl_env *env, int hid);
int irrl_mlp_eval_measured(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *mlp_w, const float *pi_w,
                           const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring, float *cmd, float *vel_his,
                           float *act_his, uint8_t *done, float *obs, float *work, const int *delay, const float *cmd_target, float a_cmd, float a_vel,
                           float a_act, const float *cmd_mean, const float *cmd_std, int clip, float *rec_obs_cond, float *rec_act_clipped,
                           float *rec_act_applied, float *rec_body, float *rec_torque, float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats,
                           const irrl_eval_scenario *scenario, const irrl_eval_kicks *kicks, const irrl_eval_gait *gait, void *hip_stream);
int irrl_mlp_eval_measured_persistent(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *mlp_w,
                                      const float *pi_w, const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring,
                                      float *cmd, float *vel_his, float *act_his, uint8_t *done, float *obs, float *work, const int *delay,
                                      const float *cmd_target, float a_cmd, float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip,
                                      float *rec_obs_cond, float *rec_act_clipped, float *rec_act_applied, float *rec_body, float *rec_torque,
                                      float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats, const irrl_eval_scenario *scenario,
                                      const irrl_eval_kicks *kicks, const irrl_eval_gait *gait, void *hip_stream);

/* ENSEMBLE ANALYSIS OF A BODY RECORDER: state-space entropy, cell counts, per-feature histograms and moments per (condition, frame) -- what the
 * reference's figure scripts do with a perturbation exploration (Data_Visualization_Code/Figure3.py:145-151 and Figure4.py:160-166 `entropy`,
 * Figure3.py:213-230 the time x value densities).  rec_body is the recorder of the evaluation loop, device f32 [rows, num_envs, 13] (base x y z,
 * quaternion w x y z, world linear velocity, world angular velocity), env index = condition * explorations + exploration.  Semantics in ONE text,
 * csrc/eval_elements.hpp: irrl_eval_ensemble_features turns a row into x = (z, roll, pitch, body-frame v_z, body-frame w_x, body-frame w_y) in
 * f64, irrl_eval_ensemble_key clips, divides by prec and TRUNCATES toward zero (the reference's astype(int): the cell around 0 is double width)
 * and packs the six cell indices into one mixed-radix key, irrl_eval_ensemble_bin is the histogram rule
 *   b = (int)floor((x - hist_lo) * (hist_bins / (hist_hi - hist_lo))),  x == hist_hi -> the last bin,  x outside [hist_lo, hist_hi] dropped.
 * For condition c and analysed frame f (row frame_first + f * frame_every of the recorder) over the explorations e whose mask byte is non-zero
 * (mask NULL: all) and whose six features are finite -- M of them --:
 *   entropy[c, f] = -sum over occupied cells of (n / M) log(n / M)  (nats; n = samples in the cell);  0 where M = 0
 *   counts[c, f]  = M | number of occupied cells | the largest n
 *   hist[c, f, i, b]   (NULL or hist_bins = 0: off) = kept samples whose UNCLIPPED feature i falls into bin b
 *   moments[c, f, i]   (NULL: off) = sum x_i | sum x_i^2 over the kept samples, unclipped, f64
 * One workgroup per (c, f) sorts the keys: entropy, counts and hist are the same bits from run to run and under any permutation of a
 * condition's explorations.  Stateless and stream-ordered, no env handle.
 * Refused before any HIP call, with "irrl_eval_ensemble" in the text: a NULL rec_body, spec or entropy; conditions * explorations != num_envs;
 * explorations outside 1 .. IRRL_EVAL_ENSEMBLE_MAX; frames < 0, frame_first < 0, frame_every < 1, frame_first + (frames - 1) * frame_every >= rows;
 * prec_i <= 0, lb_i > ub_i, a bound that is not finite or lies beyond 2^62 cells; a product of the six cell ranges of 2^63 or more; hist_bins
 * outside 0 .. IRRL_EVAL_ENSEMBLE_MAX_BINS, or hist_hi_i <= hist_lo_i with bins on.  frames == 0 is accepted and does nothing. */
#define IRRL_EVAL_ENSEMBLE_DIM 6
#define IRRL_EVAL_ENSEMBLE_MAX 16384
#define IRRL_EVAL_ENSEMBLE_MAX_BINS 256
typedef struct irrl_eval_ensemble_spec {
  double lb[6], ub[6], prec[6];
  double hist_lo[6], hist_hi[6];
  int hist_bins;
} irrl_eval_ensemble_spec;
int irrl_eval_ensemble(const float *rec_body, int rows, int num_envs, int conditions, int explorations, int frame_first, int frame_every, int frames,
                       const uint8_t *mask, const irrl_eval_ensemble_spec *spec, double *entropy, uint32_t *counts, uint32_t *hist, double *moments,
                       void *hip_stream);

/* RECURRENCE ANALYSIS OF A BODY RECORDER: per robot the time x time matrix of quantised state distances and the recurrence measures read off it
 * -- the reference's recurrence plot (Data_Visualization_Code/Figure4.py:479-570, the rule at :495-509) and, from the same distance evaluations,
 * recurrence rate, determinism, laminarity, the longest line and the recurrence count per time lag (whose first peak is the stride period).
 * rec_body as for irrl_eval_ensemble, device f32 [rows, num_envs, 13].  Semantics in ONE text, csrc/eval_elements.hpp:
 *   frame i = 0 .. frames - 1 (T = frames) of robot e is recorder row frame_first + i * frame_every;
 *   x_i = irrl_eval_ensemble_features(row), unchanged; a frame is KEPT iff its six features are finite;
 *   u_i[k] = (x_i[k] - (lb[k] + ub[k]) / 2.0) / (ub[k] - lb[k])                                (irrl_eval_recurrence_state)
 *   d2 = sum_k D_k * D_k in index order, D_k = u_i[k] - u_j[k], every product rounded on its own  (irrl_eval_recurrence_dist2)
 *   c = sqrt(d2) / eps,  q_ij = c >= steps ? steps : (int)floor(c)                             (irrl_eval_recurrence_level)
 *   a pair with a dropped frame has q = steps;  R_ij = q_ij < radius;  w = max(theiler, 1),  R'_ij = R_ij && |i - j| >= w.
 * Outputs per robot, all integers (any order of the reductions gives the same words):
 *   counts[e, 9] u32:  0 KEPT         kept frames
 *                      1 REC          pairs i < j, j - i >= w, with R_ij
 *                      2 DIAG_POINTS  those of REC on diagonal lines of length >= lmin; a diagonal line is a maximal run of consecutive i with
 *                                     R_{i,i+tau} for a fixed tau >= w, the matrix border ends a line like a non-recurrent point
 *                      3 DIAG_LINES   the number of such lines
 *                      4 DIAG_MAX     the longest diagonal line of any length, 0 if none
 *                      5 VERT_POINTS  points of R' on vertical lines of length >= vmin; a vertical line is a run over consecutive i for a fixed
 *                                     j in the FULL matrix with the band |i - j| < w removed
 *                      6 VERT_LINES   7 VERT_MAX
 *                      8 REC_FULL     points of R' over the full matrix (= 2 REC)
 *   lag[e, l] u32, l = 0 .. lags - 1 (lags <= frames; NULL or lags = 0: off) = the number of i with i + l < T and R_{i,i+l}; independent of
 *                      theiler; lag[e, 0] = KEPT
 *   matrix[s, i, j] u8 [matrix_count, T, T] (NULL or matrix_count = 0: off) = q_ij of robot matrix_env[s], the full symmetric matrix, the
 *                      diagonal 0 for kept frames and `steps` for dropped ones; a robot may be listed more than once.
 * One workgroup per robot, no global atomics, no floating-point atomics, every output word has one writer.  Stateless and stream-ordered, no env
 * handle.  frames == 0 is accepted and does nothing.
 * Refused before any HIP call, with "irrl_eval_recurrence: " in front of the text: a NULL rec_body, spec or counts; num_envs < 1; frames outside
 * 0 .. IRRL_EVAL_RECURRENCE_MAX_FRAMES; frame_first < 0, frame_every < 1, frame_first + (frames - 1) * frame_every >= rows; ub_k <= lb_k or a
 * bound that is not finite; eps <= 0 or not finite; steps outside 1 .. 255; radius outside 1 .. steps; theiler < 0, lmin < 1, vmin < 1; lags
 * outside 0 .. frames; lags > 0 with a NULL lag; matrix_count outside 0 .. IRRL_EVAL_RECURRENCE_MAX_MATRICES; matrix_count > 0 with a NULL
 * matrix; a matrix_env outside 0 .. num_envs - 1. */
#define IRRL_EVAL_RECURRENCE_MAX_FRAMES 2048
#define IRRL_EVAL_RECURRENCE_MAX_MATRICES 8
#define IRRL_EVAL_RECURRENCE_COUNTS 9
typedef struct irrl_eval_recurrence_spec {
  double lb[6], ub[6]; double eps;
  int steps, radius, theiler, lmin, vmin, lags, matrix_count;
  int matrix_env[8];
} irrl_eval_recurrence_spec;
int irrl_eval_recurrence(const float *rec_body, int rows, int num_envs, int frame_first, int frame_every, int frames,
                         const irrl_eval_recurrence_spec *spec, uint32_t *counts, uint32_t *lag, uint8_t *matrix, void *hip_stream);

/* ANALYSES OF A GAIT RECORDER: debounced footfalls per robot and leg, and the motor's torque-speed plane per (condition, joint).  Both read
 * rec_gait, device f32 [rows, num_envs, IRRL_EVAL_GAIT_REC_DIM] (tq 12 | qd 12 | in_contact 4 | f_z 4, above), and rec_done, device u8
 * [rows, num_envs] or NULL for none.  Analysed frame i = 0 .. frames - 1 is recorder row frame_first + i * frame_every.  A `done` row holds the
 * reset state, so robot e is analysed over i < T_e: T_e is the first analysed frame whose rec_done word is non-zero, `frames` if there is none.
 * Stateless and stream-ordered, no env handle; no global atomics, no floating-point atomics, every output word has one writer; the words are the
 * same bits from run to run.  Semantics in ONE text, csrc/eval_elements.hpp (irrl_eval_footfall_*, irrl_eval_motor_*).
 *
 * irrl_eval_footfall -- the reference never reads raw contact flags: Data_Visualization_Code/Figure2.py:97-116 (Contact_filtered) takes a 5-frame
 * moving average cast to bool and then fills every contact gap shorter than 10 frames.  THE FILTER RULE (irrl_eval_footfall_filter), for leg l
 * over the robot's window T = T_e with c[k] = (column 24 + l != 0):
 *   dilate: d[k] = any c[k'] with |k' - k| <= reach and 0 <= k' < T;
 *   hold:   f = d; then in increasing j = 0 .. T - hold - 2: if f[j] && !f[j+1], f[j+1] = any of f[j+1 .. j+hold].
 * With reach = 2, hold = 10 this is Contact_filtered for every T >= 5 (below 5, np.convolve(mode='same') returns five samples and the reference
 * has no defined answer).  THE CLOSED FORM the kernel uses (one writer per frame; irrl_eval_footfall_fill_end):
 *   f[k] = d[k] || (k <= T - hold - 1 && a exists && b exists && b - a <= hold),  a = the last k' < k with d[k'],  b = the first k' > k with d[k'];
 * so leading and trailing gaps are never filled, gaps of at most hold - 1 frames are filled, the last `hold` frames of a window are not filled.
 * Outputs, all integers:
 *   counts[e, leg, IRRL_EVAL_FOOTFALL_COUNTS] u32 (required):
 *      0 FRAMES          T_e
 *      1 RAW_STANCE      frames with c
 *      2 RAW_TOUCHDOWNS  k >= 1 with !c[k-1] && c[k]
 *      3 STANCE          frames with f
 *      4 TOUCHDOWNS      rising edges of f, k >= 1 with !f[k-1] && f[k]
 *      5 LIFTOFFS        falling edges of f, k >= 1 with f[k-1] && !f[k]
 *      6 FIRST_TD, 7 LAST_TD   frame index of the first / last touchdown, 0xFFFFFFFF if none
 *      8 STANCE_PHASES, 9 STANCE_SUM, 10 STANCE_MAX   complete stance phases (a touchdown and the next liftoff, both inside the window): their
 *                        number, their summed length in frames (liftoff - touchdown), the longest
 *      11 SWING_PHASES, 12 SWING_SUM, 13 SWING_MAX    complete swings (a liftoff and the next touchdown; touchdown - liftoff)
 *      the stride period in frames is (LAST_TD - FIRST_TD) / (TOUCHDOWNS - 1)
 *   support[e, 16] u32 (NULL: off)  the frames i < T_e whose support pattern p = sum_l f_l << l has that value; support[e, 0] is flight
 *   phase[e, 3, phase_bins] u32 (NULL or phase_bins = 0: off)  for leg l = 1 .. 3 every touchdown of leg l at frame t with a <= t < b, a and b
 *                        consecutive touchdowns of leg 0, counted in bin (t - a) * phase_bins / (b - a) (integer division) of row l - 1; touchdowns
 *                        outside a complete stride of leg 0 are not counted
 *   pattern[i, e] u8 [frames, num_envs] (NULL: off)  p of frame i, 0 for i >= T_e: the gait diagram
 * One workgroup per robot; the flags live in LDS as 64-frame bit words.
 *
 * irrl_eval_motor_plane -- the reference's Figure 5 (Data_Visualization_Code/Figure5.py:250-289, :379-392): where the joints operate against
 * the motor envelope, and the stride-folded torque-speed loop.  env index = condition * robots + robot.  THE SAMPLE of robot r, frame i < T_e,
 * joint j (irrl_eval_motor_sample): ratio = (j % 3 == 2) ? knee_ratio : 1.0, m = (double)tq_j / ratio, w = (double)qd_j * ratio, kept iff both are
 * finite.  THE ENVELOPE (irrl_eval_motor_up, the f64 restatement of the env's torque clamp):
 *   up(w) = w > w_crit ? tau_max - (w - w_crit) * (tau_max / (w_max - w_crit)) : tau_max,   low(w) = -up(-w),  every product rounded on its own.
 * Outputs:
 *   counts[c, 12, IRRL_EVAL_MOTOR_COUNTS] u32 (required):  0 SAMPLES  1 SAT_UP (m >= up(w) - sat)  2 SAT_LOW (m <= low(w) + sat)
 *      3 OUTSIDE (m > up(w) + sat || m < low(w) - sat)  4 MOTORING (m * w > 0)  5 BRAKING (m * w < 0)
 *   hist[c, 12, t_bins, w_bins] u32 (NULL or a zero bin count: off)  the kept samples by irrl_eval_ensemble_bin(m, t_lo, t_hi, t_bins) and
 *      irrl_eval_ensemble_bin(w, w_lo, w_hi, w_bins); a sample outside either range is dropped from hist only
 *   fold[c, 12, period, 3] f64 (NULL or period = 0: off)  the count, sum of m and sum of w of the kept samples with i % period == p, added robot by
 *      robot in index order and, within a robot, frame by frame in index order: the same bits on every machine (the reference's phase_jagged fold)
 * One workgroup per (condition, joint); the 2-D histogram in LDS with integer LDS atomics; one thread per phase p walks its samples in order.
 *
 * Both refuse before any HIP call, with "irrl_eval_footfall: " / "irrl_eval_motor_plane: " in front of the text: a NULL rec_gait, spec or counts;
 * num_envs < 1; frames outside 0 .. the limit; frame_first < 0, frame_every < 1, frame_first + (frames - 1) * frame_every >= rows; reach outside
 * 0 .. IRRL_EVAL_FOOTFALL_MAX_REACH, hold outside 0 .. IRRL_EVAL_FOOTFALL_MAX_HOLD, phase_bins outside 0 .. IRRL_EVAL_FOOTFALL_MAX_BINS; t_bins or
 * w_bins outside 0 .. IRRL_EVAL_MOTOR_MAX_BINS, period outside 0 .. IRRL_EVAL_MOTOR_MAX_PERIOD; w_max <= w_crit; tau_max, w_crit, w_max,
 * knee_ratio or sat not finite, tau_max <= 0, knee_ratio <= 0, sat < 0; t_hi <= t_lo or w_hi <= w_lo (or a bound not finite) with bins on;
 * robots < 1, conditions < 1, conditions * robots != num_envs.  frames == 0 is accepted and does nothing. */
#define IRRL_EVAL_FOOTFALL_MAX_FRAMES 16384
#define IRRL_EVAL_FOOTFALL_MAX_REACH 8
#define IRRL_EVAL_FOOTFALL_MAX_HOLD 64
#define IRRL_EVAL_FOOTFALL_MAX_BINS 64
#define IRRL_EVAL_FOOTFALL_COUNTS 14
#define IRRL_EVAL_FOOTFALL_NONE 0xFFFFFFFFu
enum {
  IRRL_EVAL_FOOTFALL_FRAMES = 0, IRRL_EVAL_FOOTFALL_RAW_STANCE, IRRL_EVAL_FOOTFALL_RAW_TOUCHDOWNS, IRRL_EVAL_FOOTFALL_STANCE,
  IRRL_EVAL_FOOTFALL_TOUCHDOWNS, IRRL_EVAL_FOOTFALL_LIFTOFFS, IRRL_EVAL_FOOTFALL_FIRST_TD, IRRL_EVAL_FOOTFALL_LAST_TD,
  IRRL_EVAL_FOOTFALL_STANCE_PHASES, IRRL_EVAL_FOOTFALL_STANCE_SUM, IRRL_EVAL_FOOTFALL_STANCE_MAX,
  IRRL_EVAL_FOOTFALL_SWING_PHASES, IRRL_EVAL_FOOTFALL_SWING_SUM, IRRL_EVAL_FOOTFALL_SWING_MAX
};
typedef struct irrl_eval_footfall_spec {
  int reach, hold, phase_bins;
} irrl_eval_footfall_spec;
int irrl_eval_footfall(const float *rec_gait, const uint8_t *rec_done, int rows, int num_envs, int frame_first, int frame_every, int frames,
                       const irrl_eval_footfall_spec *spec, uint32_t *counts, uint32_t *support, uint32_t *phase, uint8_t *pattern, void *hip_stream);

#define IRRL_EVAL_MOTOR_MAX_FRAMES 16384
#define IRRL_EVAL_MOTOR_MAX_BINS 64
#define IRRL_EVAL_MOTOR_MAX_PERIOD 1024
#define IRRL_EVAL_MOTOR_COUNTS 6
enum {
  IRRL_EVAL_MOTOR_SAMPLES = 0, IRRL_EVAL_MOTOR_SAT_UP, IRRL_EVAL_MOTOR_SAT_LOW, IRRL_EVAL_MOTOR_OUTSIDE, IRRL_EVAL_MOTOR_MOTORING, IRRL_EVAL_MOTOR_BRAKING
};
typedef struct irrl_eval_motor_spec {
  double tau_max, w_crit, w_max, knee_ratio, sat, t_lo, t_hi, w_lo, w_hi;
  int t_bins, w_bins, period;
} irrl_eval_motor_spec;
int irrl_eval_motor_plane(const float *rec_gait, const uint8_t *rec_done, int rows, int num_envs, int conditions, int robots, int frame_first,
                          int frame_every, int frames, const irrl_eval_motor_spec *spec, uint32_t *counts, uint32_t *hist, double *fold,
                          void *hip_stream);

/* TRACE RECORDERS OF THE FIVE-LAUNCH EVALUATION LOOP: what the policy holds inside, per control step (the reference's `--corr` path records
 * CustomerLstmNN.get_hidden_state after every predict, run_bp_v5.py:458-460; its `--val` path the critic's value).  irrl_eval_trace is a HOST
 * struct of device pointers, each may be NULL (but not both):
 *   rec_lstm  f32 [steps, N, 4 * hid]  the ACTOR's half of lstm_state, c0 | h0 | c1 | h1 (lstm_state[:, 0 : 4 hid]), AFTER step k's policy step:
 *                                      row k holds the state that has consumed step k's observation, reset included where `done` was set
 *   rec_value f32 [steps, N]           the critic's value of step k (the `value` column of the work array)
 * irrl_lstm_eval_traced is irrl_lstm_eval_measured with the struct behind `gait`; irrl_mlp_eval_traced is irrl_mlp_eval_measured with it, and
 * refuses rec_lstm: MlpPolicy has no recurrent state.  With a trace the loop makes ONE extra launch per step between the policy step and the action
 * filter (irrl_eval_trace_kernel, csrc/eval_rollout.hpp: a lane per (env, column), both copies coalesced); trace == NULL is the measured call,
 * launch for launch.  Every other buffer is bit-identical to the call without the trace.  There is NO persistent form: the persistent kernel
 * keeps the state in LDS that is full, and does not run the critic at all.
 * Errors (non-zero, irrl_last_error() set with the entry point's own name, checked before any HIP call): the refusals of the measured calls;
 * a trace whose two pointers are both NULL; rec_lstm with irrl_mlp_eval_traced. */
typedef struct irrl_eval_trace {
  float *rec_lstm;
  float *rec_value;
} irrl_eval_trace;
int irrl_lstm_eval_traced(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *lstm_w, const float *pi_w,
                          const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring, float *cmd, float *vel_his,
                          float *act_his, float *lstm_state, uint8_t *done, float *obs, float *work, const int *delay, const float *cmd_target, float a_cmd,
                          float a_vel, float a_act, const float *cmd_mean, const float *cmd_std, int clip, float *rec_obs_cond, float *rec_act_clipped,
                          float *rec_act_applied, float *rec_body, float *rec_torque, float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats,
                          const irrl_eval_scenario *scenario, const irrl_eval_kicks *kicks, const irrl_eval_gait *gait, const irrl_eval_trace *trace,
                          void *hip_stream);
int irrl_mlp_eval_traced(irrl_env *env, int steps, long long step0, int hid, int ob_dim, int act_dim, const float *const *mlp_w, const float *pi_w,
                         const float *pi_b, const float *vf_w, const float *vf_b, const float *logstd, int depth, float *ring, float *cmd, float *vel_his,
                         float *act_his, uint8_t *done, float *obs, float *work, const int *delay, const float *cmd_target, float a_cmd, float a_vel,
                         float a_act, const float *cmd_mean, const float *cmd_std, int clip, float *rec_obs_cond, float *rec_act_clipped,
                         float *rec_act_applied, float *rec_body, float *rec_torque, float *rec_obs_raw, float *rec_reward, uint8_t *rec_done, double *stats,
                         const irrl_eval_scenario *scenario, const irrl_eval_kicks *kicks, const irrl_eval_gait *gait, const irrl_eval_trace *trace,
                         void *hip_stream);

/* CORRELATION MOMENTS OF TWO RECORDER WINDOWS: the sums a Pearson correlation (or a covariance, or a PCA) of recorder columns needs -- the
 * reference's `--corr` figure, contact flags x LSTM units (run_bp_v5.py:1032-1088), and its full df.corr().  x is device f32 [rows, num_envs,
 * x_dim], of which the columns x_first .. x_first + x_count are analysed; y the same with its own three numbers; x and y may be the same buffer
 * and window.  Frames and T_e are irrl_eval_motor_plane's: analysed frame i is recorder row irrl_eval_recurrence_row(frame_first, frame_every, i),
 * T_e = the first analysed frame whose rec_done word is non-zero (rec_done NULL: T_e = frames); env index = condition * robots + robot, per-robot
 * matrices are conditions = num_envs, robots = 1.  Outputs per condition g over the samples i < T_e of its robots:
 *   count[g] i64            sum of T_e
 *   sx[g, cx, 2] f64        sum x, sum x^2          sy[g, cy, 2] f64   the same of y
 *   sxy[g, cx, cy] f64      sum x y
 *   range_x[g, cx, 2] f32, range_y[g, cy, 2] f32 (NULL: off)   min, max over the pooled samples, (+inf, -inf) when there are none: what tells a
 *                           constant column EXACTLY (n sum x^2 - (sum x)^2 is not to be trusted to be 0)
 * THE ONE ORDER (csrc/eval_elements.hpp irrl_eval_corr_add): per robot every accumulator starts at +0.0 and takes its frames in ascending order
 * as s = s + (double)a * (double)b (sum x: b = 1); the condition's total starts at +0.0 and takes its robots' partials in ascending robot order.
 * The product of two f32 is exact in f64, so a fused multiply-add and a multiply and an add give the same bits: device, host and numpy agree bit
 * for bit.  No atomics; nothing depends on the order in which waves arrive.  min / max keep m unless v < m (v > m): a NaN sample never enters a
 * range.  A non-finite sample poisons the accumulators of its own column (pairs) and no other.
 * work: device f64 [irrl_eval_correlation_work(num_envs, spec)] = num_envs * (cx cy + 3 cx + 3 cy + 1) doubles, the robots' partials; needed with
 * robots > 1, may be NULL with robots == 1 (the first kernel then writes the outputs itself).  irrl_eval_correlation_work needs no GPU; 0 for a
 * NULL or refused spec or num_envs < 1.
 * Refused before any HIP call with "irrl_eval_correlation: " in front of the text: NULL x, y, spec, count, sx, sy or sxy; x_dim or y_dim < 1, a
 * window outside its row width; x_count outside 1 .. IRRL_EVAL_CORR_MAX_X; y_count outside 1 .. IRRL_EVAL_CORR_MAX_Y; num_envs < 1, conditions or
 * robots < 1, conditions * robots != num_envs; frames outside 1 .. IRRL_EVAL_CORR_MAX_FRAMES; frame_first < 0, frame_every < 1, frame_first +
 * (frames - 1) * frame_every >= rows; robots > 1 with work NULL. */
#define IRRL_EVAL_CORR_MAX_FRAMES 16384
#define IRRL_EVAL_CORR_MAX_X 64
#define IRRL_EVAL_CORR_MAX_Y 1024
typedef struct irrl_eval_corr_spec {
  int x_dim, x_first, x_count, y_dim, y_first, y_count;
} irrl_eval_corr_spec;
size_t irrl_eval_correlation_work(int num_envs, const irrl_eval_corr_spec *spec);
int irrl_eval_correlation(const float *x, const float *y, const uint8_t *rec_done, int rows, int num_envs, int conditions, int robots,
                          int frame_first, int frame_every, int frames, const irrl_eval_corr_spec *spec, int64_t *count, double *sx, double *sy,
                          double *sxy, float *range_x, float *range_y, double *work, void *hip_stream);

/* SPECTROGRAM AND WELCH SPECTRUM OF RECORDER COLUMNS: the reference's `--virba`, its "time-frequency spectrum analysis of output"
 * (run_bp_v5.py:1090-1117): scipy.signal.spectrogram(column, 1 / control_dt) of the joint angles, joint rates and actions -- whether a policy
 * chatters, at which frequency, and where delay and the low-pass filters move that energy.  x is device f32 [rows, num_envs, x_dim], of which
 * the columns x_first .. x_first + x_count are analysed.  Frames and T_e are irrl_eval_correlation's: analysed frame i is recorder row
 * irrl_eval_recurrence_row(frame_first, frame_every, i), T_e = the first analysed frame whose rec_done word is non-zero (rec_done NULL or no such
 * word: T_e = frames); env index = condition * robots + robot.
 * Segment s of robot e covers the frames s * hop .. s * hop + nperseg - 1 and exists iff it lies wholly inside i < T_e:
 * S_e = T_e >= nperseg ? (T_e - nperseg) / hop + 1 : 0 -- a robot that terminates early gives fewer segments, the reset row enters none.
 * THE ONE ORDER (csrc/eval_elements.hpp irrl_eval_spectrum_*), all in f64, per segment and column c:
 *   v_n = (double)x_n * scale[c];  detrend == 1: m = (((0.0 + v_0) + v_1) + ...) / nperseg, v_n -= m (detrend == 0: nothing is subtracted);
 *   a_n = v_n * window[n];  Re_k = sum_n a_n * tw[(k n) mod nperseg].cos,  Im_k = -sum_n a_n * tw[(k n) mod nperseg].sin, n ascending from +0.0,
 *   k = 0 .. K - 1, K = nperseg / 2 + 1;  P_k = g_k * density * (Re_k^2 + Im_k^2), density = 1 / (fs * sum_n window[n]^2), g_k = 2 except g_0 = 1
 *   and, with an even nperseg, g_{K-1} = 1.
 * This is scipy.signal.spectrogram(mode='psd', scaling='density', return_onesided=True, nfft=nperseg, noverlap=nperseg - hop); nperseg = 256,
 * hop = 224, detrend = 1 and the Tukey(0.25) window are the reference's bare call.  The DFT is direct (nperseg need not be a power of two): a
 * length-n dot product errs by at most n 2^-53 sum |a_n|, whatever the order and whether fused, which is what the tests' bound rests on.
 * Tables, both device f64, owned by the caller: window [nperseg]; tw [nperseg, 2] = cos, sin of 2 pi j / nperseg.  irrl_eval_spectrum_tables
 * fills HOST copies without touching the GPU, so that device, host program, numpy twin and tests share the same table bits: window_kind
 * 0 boxcar (ones), 1 Hann, periodic (scipy get_window('hann', n)): 0.5 - 0.5 cos(2 pi n / nperseg), 2 Tukey(alpha), periodic (scipy
 * get_window(('tukey', alpha), n)): with M = nperseg + 1 and width = floor(alpha (M - 1) / 2) the samples n <= width are
 * 0.5 (1 + cos(pi (-1 + 2 n / alpha / (M - 1)))), the samples n >= M - width - 1 are 0.5 (1 + cos(pi (-2 / alpha + 1 + 2 n / alpha / (M - 1)))), the
 * rest 1, the last of the M dropped; alpha <= 0 is the boxcar, alpha >= 1 Hann.  -> 0, or non-zero with "irrl_eval_spectrum_tables: " in front of
 * the text for a NULL table, nperseg outside 8 .. IRRL_EVAL_SPECTRUM_MAX_NPERSEG, a window_kind outside 0 .. 2 or an alpha that is not finite.
 * Outputs, K = nperseg / 2 + 1:
 *   segments[g] i64             the sum of S_e over the condition's robots
 *   psd_sum[g, cx, K] f64       the sum of P_k over those segments: per robot in ascending segment order from +0.0, then the robots' partials in
 *                               ascending robot order from +0.0.  The Welch spectrum is psd_sum / segments (sums, not means, like the moments)
 *   sxx[m, cx, S_max, K] f64    (NULL or matrix_count = 0: off) S_max = (frames - nperseg) / hop + 1: the P_k of every segment of robot
 *                               matrix_env[m] -- the reference's pcolormesh --, segments >= S_e written as 0; a robot may be listed more than once
 * work: device f64 [irrl_eval_spectrum_work(num_envs, spec)] = num_envs * (cx K + 1) doubles: the robots' partials [num_envs, cx, K], then S_e as
 * int64 [num_envs]; needed with robots > 1, may be NULL with robots == 1 (the first kernel then writes the outputs itself).
 * irrl_eval_spectrum_work needs no GPU; 0 for a NULL or refused spec or num_envs < 1.
 * No atomics on any output, every output word has one writer, the same bits from run to run.  A non-finite sample poisons the bins of its own
 * column in its own segment(s) and the psd_sum of its condition, and nothing else.  Stateless and stream-ordered, no env handle.
 * frames < nperseg is accepted: nothing is launched, segments and psd_sum are set to zero (device memory by a memset on the stream; memory HIP
 * does not know as a device's is written by the host), no error is set.
 * Refused before any HIP call with "irrl_eval_spectrum: " in front of the text: NULL x, spec, window, tw, segments or psd_sum; x_dim < 1, a window
 * outside its row width; x_count outside 1 .. IRRL_EVAL_SPECTRUM_MAX_X; nperseg outside 8 .. IRRL_EVAL_SPECTRUM_MAX_NPERSEG; hop outside
 * 1 .. nperseg; detrend outside 0 .. 1; fs or a used scale entry that is not finite or <= 0; matrix_count outside 0 ..
 * IRRL_EVAL_SPECTRUM_MAX_MATRICES; matrix_count > 0 with a NULL sxx; a matrix_env outside 0 .. num_envs - 1; num_envs < 1, conditions or robots
 * < 1, conditions * robots != num_envs; frames outside 1 .. IRRL_EVAL_SPECTRUM_MAX_FRAMES; frame_first < 0, frame_every < 1, frame_first +
 * (frames - 1) * frame_every >= rows; robots > 1 with work NULL. */
#define IRRL_EVAL_SPECTRUM_MAX_FRAMES 16384
#define IRRL_EVAL_SPECTRUM_MAX_X 64
#define IRRL_EVAL_SPECTRUM_MAX_NPERSEG 1024
#define IRRL_EVAL_SPECTRUM_MAX_MATRICES 8
typedef struct irrl_eval_spectrum_spec {
  int x_dim, x_first, x_count, nperseg, hop, detrend, matrix_count;
  int matrix_env[8];
  double fs;
  double scale[64];
} irrl_eval_spectrum_spec;
int irrl_eval_spectrum_tables(int nperseg, int window_kind, double alpha, double *window, double *tw);
size_t irrl_eval_spectrum_work(int num_envs, const irrl_eval_spectrum_spec *spec);
int irrl_eval_spectrum(const float *x, const uint8_t *rec_done, int rows, int num_envs, int conditions, int robots, int frame_first,
                       int frame_every, int frames, const irrl_eval_spectrum_spec *spec, const double *window, const double *tw,
                       int64_t *segments, double *psd_sum, double *sxx, double *work, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
