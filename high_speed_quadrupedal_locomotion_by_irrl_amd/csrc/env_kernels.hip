// env_kernels.hip -- __global__ wrappers of the lane bodies in env_core.hpp (gfx950 only); compiled once per lane layout (build.py).
// Launch shape of the lane kernels: 64-thread workgroups = one wave = 4 robots (16 lanes per robot, one DPP row each: pools of up to one wave per SIMD, 4096 robots on an MI355X) or 16 robots
// (4 lanes per robot, one DPP quad each).  At N = 4096 the 16-lane layout is 1024 workgroups -> one wave on every SIMD of the 256 CUs; the kernels
// keep the whole robot state in registers across the 8 substeps (no LDS; scratch only in the reset branch), so __launch_bounds__(256, 1) lets the
// allocator use the full 512-register budget of a SIMD that hosts a single wave.  The rollout kernels (policy in the same launch) run 256-thread
// workgroups: four env waves = 16 robots per workgroup.
#ifndef IRRL_LANES_PER_ROBOT
#define IRRL_LANES_PER_ROBOT 16
#endif
#if IRRL_LANES_PER_ROBOT == 16
#include "lanes_hip16.hpp"
#define IRRL_ROBOTS_PER_WAVE 4
#else
#include "lanes_hip.hpp"
#define IRRL_ROBOTS_PER_WAVE 16
#endif
#include "env_core.hpp"
// second instantiation of the lane bodies with the meteorite (Crutial: True) compiled out: pools without it -- every benchmark
// and training configuration -- run the step kernel built from this one (measured: the run-time-flag version costs 0.5 us of
// the 38 us step even with the flag off: 16 more VGPRs live across the substeps and the branches in the schedule)
#undef IRRL_CORE_NS
#undef IRRL_CRUTIAL
#define IRRL_CORE_NS irrl_plain
#define IRRL_CRUTIAL(P) false
#include "env_core.hpp"

#if IRRL_LANES_PER_ROBOT == 16
#include "policy_step.hpp"   // the LSTM policy's rollout step (device code shared with lstm_kernels.hip)
#endif
#if defined(IRRL_EVAL_UNIT) || defined(IRRL_EVAL_MLP_UNIT)
#include "eval_elements.hpp"   // the evaluation loop's per-element arithmetic and its argument block (shared with eval_rollout.hpp)
#endif
#include "env_kernels_decl.h"   // every kernel below is declared there: the launcher (irrl_env_abi.hip) sees the same signatures

// This file is compiled six times (build.py; three of them hold the rollout / evaluation kernels alone, see below): once per lane layout, kernel names suffixed _l16 / _l4, and the 4-lane layout once more for
// TWO waves per SIMD (_l4w2, -DIRRL_L4_WAVES2: 256 registers per wave, ~130-220 of the step kernels' values in scratch).  Pools of more than
// 16 384 robots are more 4-lane waves than the chip has SIMDs; two resident waves issue 1.35 x what one does (HISTORY.md Appendix C, 2a), which
// pays for the spills: 32 768 envs 394 -> 450 M env-steps/s, 131 072 envs 394 -> 482 M, 16 384 envs (one wave per SIMD either way) 393 -> 386 M
// -- the launcher takes _l4w2 above 16 384 robots only (profiles/r06_ab_l4_two_waves_per_simd_same_box.log).  Same source, same arithmetic.
#if IRRL_LANES_PER_ROBOT == 16
#define IRRL_K(name) name##_l16
#elif defined(IRRL_L4_WAVES2)
#define IRRL_K(name) name##_l4w2
#else
#define IRRL_K(name) name##_l4
#endif

// XCD-aware block -> robots mapping.  The hardware hands consecutive workgroups to the 8 XCDs round-robin (workgroup b runs on XCD
// b % 8), and every XCD has its own L2.  With the identity mapping the four robots of workgroup b and those of b + 1 -- neighbours
// in every array of the pool, 16 B apart in a per-env scalar array -- sit on different XCDs, so one 128-byte line is fetched from
// HBM by up to eight L2s.  irrl_xcd_block() renumbers the blocks so that XCD x owns ONE contiguous range of robots (a bijection of
// [0, gridDim.x) for any grid size): a line is then fetched by one L2 (two at a range boundary).  Results do not change -- only
// which wave computes which robot.
__device__ __forceinline__ int irrl_xcd_block() {
#ifdef IRRL_NO_XCD_SWIZZLE   /* A/B switch of tools/build_variants.py */
  return (int)blockIdx.x;
#endif
  const int nb = (int)gridDim.x, b = (int)blockIdx.x;
  const int x = b & 7, j = b >> 3;                  // XCD of this workgroup, its rank among that XCD's workgroups
  const int q = nb >> 3, r = nb & 7;                // XCD x gets q workgroups, + 1 if x < r
  return x * q + (x < r ? x : r) + j;
}
// The lane context: which robot and leg a lane integrates.  env: the robot; rw: its index inside the wave; leg: the lane's leg; valid: this
// lane owns the stores of (robot, leg) -- with 16 lanes per robot that is sub-lane 0 of each quad.  Idle rows (quads) shadow the last robot
// with their stores masked.  `wave`: the wave's index in the pool (a kernel decides how its workgroups map to it), `lane`: 0 .. 63.
struct LaneCtx { int env, rw, leg; bool valid; };
__device__ __forceinline__ LaneCtx irrl_lane_ctx(const EnvParams &P, int wave, int lane) {
  LaneCtx c;
#if IRRL_LANES_PER_ROBOT == 16
  c.rw = lane >> 4; c.env = wave * 4 + c.rw; c.leg = (lane >> 2) & 3;
  c.valid = (c.env < P.n_envs) && ((lane & 3) == 0);
#else
  c.rw = lane >> 2; c.env = wave * 16 + c.rw; c.leg = lane & 3;
  c.valid = c.env < P.n_envs;
#endif
  if (c.env >= P.n_envs) c.env = P.n_envs - 1;
  return c;
}
// `lc` of the stand-alone lane kernels (any workgroup size); BLK: the (renumbered) block index
#define IRRL_LANE_PROLOGUE_B(BLK) \
  const LaneCtx lc = irrl_lane_ctx(P, (int)((BLK) * (blockDim.x >> 6) + (threadIdx.x >> 6)), (int)(threadIdx.x & 63u));
// P / S of a kernel body: the by-value arguments named in the kernarg segment (lanes_hip*.hpp: their fields are read where they are used,
// with scalar loads, instead of all at the kernel's entry) -- or, A/B switch of tools/build_variants.py, the arguments themselves
#ifndef IRRL_NO_PARAMS_KERNARG
#define IRRL_BIND_ARGS                                         \
  const EnvParams &P = irrl_kernarg<EnvParams>(0);             \
  const EnvState &S = irrl_kernarg<EnvState>((unsigned)((sizeof(EnvParams) + alignof(EnvState) - 1) / alignof(EnvState) * alignof(EnvState)));
#define IRRL_PARAMS_REFRESH(P) irrl_refresh(P)          /* once per step of the multi-step kernels */
// the rollout kernels' PolicyStepArgs (behind P, S and NPTR pointers): A0 names it, the multi-step kernels take a step's own copy from it per step
#define IRRL_KERNARG_ALIGN(off, T) (((off) + alignof(T) - 1) / alignof(T) * alignof(T))
#define IRRL_BIND_POLICY_ARGS_N(A0, A_, NPTR)                                                                                      \
  const PolicyStepArgs &A0 = irrl_kernarg<PolicyStepArgs>((unsigned)IRRL_KERNARG_ALIGN(                                            \
      IRRL_KERNARG_ALIGN(sizeof(EnvParams), EnvState) + sizeof(EnvState) + (NPTR) * sizeof(void *), PolicyStepArgs));
#define IRRL_BIND_POLICY_ARGS(A0, A_) IRRL_BIND_POLICY_ARGS_N(A0, A_, 4)
// the evaluation kernel's EvalArgs, the argument behind its PolicyStepArgs (behind P, S and four pointers)
#define IRRL_BIND_EVAL_ARGS(E0, E_)                                                                                                \
  const EvalArgs &E0 = irrl_kernarg<EvalArgs>((unsigned)IRRL_KERNARG_ALIGN(                                                        \
      IRRL_KERNARG_ALIGN(IRRL_KERNARG_ALIGN(sizeof(EnvParams), EnvState) + sizeof(EnvState) + 4 * sizeof(void *), PolicyStepArgs) + \
          sizeof(PolicyStepArgs), EvalArgs));
#else
#define IRRL_BIND_ARGS const EnvParams &P = P_; const EnvState &S = S_;
#define IRRL_PARAMS_REFRESH(P) (P)
#define IRRL_BIND_POLICY_ARGS_N(A0, A_, NPTR) const PolicyStepArgs &A0 = A_;
#define IRRL_BIND_POLICY_ARGS(A0, A_) IRRL_BIND_POLICY_ARGS_N(A0, A_, 4)
#define IRRL_BIND_EVAL_ARGS(E0, E_) const EvalArgs &E0 = E_;
#endif
#define IRRL_LANE_PROLOGUE IRRL_LANE_PROLOGUE_B(irrl_xcd_block())          /* the stand-alone lane kernels */
#define IRRL_LANE_PROLOGUE_IDENTITY IRRL_LANE_PROLOGUE_B((int)blockIdx.x)  /* kernels whose policy part addresses robots by blockIdx */

// one wave per SIMD and its whole register file -- or (_l4w2, above) two waves per SIMD at 256 registers each
#if defined(IRRL_L4_WAVES2) && IRRL_LANES_PER_ROBOT == 4
#define IRRL_ENV_BOUNDS __launch_bounds__(256, 2)
#else
#define IRRL_ENV_BOUNDS __launch_bounds__(256, 1)
#endif

// the multi-step kernels' closing store of the lane context they carried in registers
__device__ __forceinline__ void irrl_store_lane_back(const EnvParams &P, const EnvState &S, int env, int leg, bool valid, const irrl_plain::EnvLane &L) {
  IRRL_SUB0_ONLY_BEGIN
  irrl_plain::store_lane(IRRL_PARAMS_REFRESH(P), IRRL_PARAMS_REFRESH(S), env, leg, valid, L, P.randomize_per_episode != 0);
  IRRL_SUB0_ONLY_END
}

#if IRRL_LANES_PER_ROBOT == 16
// The persistent rollout kernels: what a step's PolicyStepArgs take from the launch's besides the fields themselves, read once in front of the step loop ...
struct PolicyStepBase {
  const float *states_first, *noise0;
  long long row0, rng0;
  size_t noise_stride;
  __device__ __forceinline__ explicit PolicyStepBase(const PolicyStepArgs &a)
      : states_first(a.states_in), noise0(a.noise), row0(a.row), rng0(a.rng_step), noise_stride((size_t)a.N * (size_t)a.act_dim) {}
  // ... and step k's arguments: the launch's, re-read inside the step, with the row, RNG step, noise row and recurrent state of step k
  __device__ __forceinline__ PolicyStepArgs at(const PolicyStepArgs &a, int k) const {
    PolicyStepArgs ak = IRRL_PARAMS_REFRESH(a);
    ak.row = row0 + k; ak.rng_step = rng0 + k;
    ak.noise = noise0 ? noise0 + (size_t)k * noise_stride : nullptr;
    ak.states_in = k == 0 ? states_first : a.states_out;
    return ak;
  }
};
#endif

#ifdef IRRL_EVAL_UNIT
// FIFTH COMPILATION (build.py, 16-lane layout): nothing but the persistent evaluation kernel (env_eval_kernels.hpp) in its two solver forms --
// RULE IRRL_RULE_SHIPPED gives irrl_eval_persistent_kernel_l16, RULE 1 (settings read from EnvParams) irrl_eval_persistent_kernel_rt_l16.  A unit
// of its own for the reason the run-time-solver twins below have one: a second caller of the policy bodies inside an existing unit changes the
// schedule of the shipped kernels there, and those are held to their ISA.
#if IRRL_LANES_PER_ROBOT != 16
#error "the evaluation kernel exists in the 16-lane layout only"
#endif
extern "C" {
#define IRRL_RK(name) name##_l16
#define IRRL_ROLLOUT_RULE IRRL_RULE_SHIPPED
#include "env_eval_kernels.hpp"
#undef IRRL_RK
#undef IRRL_ROLLOUT_RULE
#define IRRL_RK(name) name##_rt_l16
#define IRRL_ROLLOUT_RULE 1
#include "env_eval_kernels.hpp"
#undef IRRL_RK
#undef IRRL_ROLLOUT_RULE
}  // extern "C"
#elif defined(IRRL_EVAL_MLP_UNIT)
// SIXTH COMPILATION (build.py, 16-lane layout): nothing but the persistent evaluation kernel with MlpPolicy as the actor (env_eval_mlp_kernels.hpp)
// in its two solver forms -- irrl_eval_mlp_persistent_kernel_l16 and irrl_eval_mlp_persistent_kernel_rt_l16.  A unit of its own for the reason
// above: mlp_policy_wave_body would get a second caller in whichever unit took this kernel in.
#if IRRL_LANES_PER_ROBOT != 16
#error "the evaluation kernel exists in the 16-lane layout only"
#endif
extern "C" {
#define IRRL_RK(name) name##_l16
#define IRRL_ROLLOUT_RULE IRRL_RULE_SHIPPED
#include "env_eval_mlp_kernels.hpp"
#undef IRRL_RK
#undef IRRL_ROLLOUT_RULE
#define IRRL_RK(name) name##_rt_l16
#define IRRL_ROLLOUT_RULE 1
#include "env_eval_mlp_kernels.hpp"
#undef IRRL_RK
#undef IRRL_ROLLOUT_RULE
}  // extern "C"
#elif defined(IRRL_ROLLOUT_RT_UNIT)
// FOURTH COMPILATION (build.py, 16-lane layout): nothing but the run-time-solver twins of the kernels that run the policy in the same launch --
// env_rollout_kernels.hpp with RULE 1, the published rule with contact_jacobi / contact_exit / contact_tol / contact_iters / loop_count / terrain
// read from EnvParams: pools whose config has no Contact* keys, ContactSolver 1, another sweep cap or exit test, or a control step of other than
// eight substeps (the launcher's SV_MD).  A unit of their own, because next to the shipped kernels they change THOSE: the policy bodies
// (policy_step.hpp) then have two callers each instead of one, the inliner takes them in another order, and three shipped kernels held to their
// ISA come out with another schedule and register assignment (measured: actor, actor-wave and MLP rollout kernels, 17-18 k lines each).
#if IRRL_LANES_PER_ROBOT != 16
#error "the rollout kernels exist in the 16-lane layout only"
#endif
extern "C" {
#define IRRL_RK(name) name##_rt_l16
#define IRRL_ROLLOUT_RULE 1
#include "env_rollout_kernels.hpp"
#undef IRRL_RK
#undef IRRL_ROLLOUT_RULE
}  // extern "C"
#else

extern "C" {

// The step kernel exists once per (Crutial, per-contact rule): the launcher picks by EnvParams::crutial / ::contact_rule.  Suffix
// _md = the published maximum-dissipation rule of RaiSim's solver (ContactSolver bit 0, the shipped default), none = the build's
// first sliding rule.  (One kernel deciding by a run-time flag cost the OTHER rule's path 6 us of a 37 us step: both rules'
// per-substep constants were live across the sweep loop and the allocator paid for them in AGPR copies.)
#define IRRL_STEP_KERNEL(NAME, NS, RULE)                                                                                           \
  __global__ void IRRL_ENV_BOUNDS                                                                                        \
  IRRL_K(NAME)(EnvParams P_, EnvState S_, const float *action, float *ob, float *reward, uint8_t *done, float *extra) {             \
    IRRL_BIND_ARGS                                                                                                                 \
    IRRL_LANE_PROLOGUE                                                                                                             \
    NS::step_body<RULE>(P, S, lc.env, lc.leg, lc.valid, action, ob, reward, done, extra);                                          \
  }
IRRL_STEP_KERNEL(irrl_step_kernel_crutial, irrl, 0)
IRRL_STEP_KERNEL(irrl_step_kernel_crutial_md, irrl, 1)
IRRL_STEP_KERNEL(irrl_step_kernel_dir, irrl_plain, 0)
IRRL_STEP_KERNEL(irrl_step_kernel_flat, irrl_plain, IRRL_RULE_SHIPPED_FLAT)   // the default pool on flat ground (env_core.hpp IRRL_FLAT_GROUND)
IRRL_STEP_KERNEL(irrl_step_kernel_md, irrl_plain, 1)   // the published rule under the other solver settings (Gauss-Seidel order / confirming exit)

// the default pool: no meteorite, published rule
__global__ void IRRL_ENV_BOUNDS
IRRL_K(irrl_step_kernel)(EnvParams P_, EnvState S_, const float *action, float *ob, float *reward, uint8_t *done, float *extra) {
  IRRL_BIND_ARGS
  IRRL_LANE_PROLOGUE
#ifdef IRRL_PROFILE_WAVES   /* diagnostic build (tools/wave_spread.py): extra[env][5] <- this wave's duration in 100 MHz ticks */
  const unsigned long long t0_ = wall_clock64();
#endif
  irrl_plain::step_body<IRRL_RULE_SHIPPED>(P, S, lc.env, lc.leg, lc.valid, action, ob, reward, done, extra);
#ifdef IRRL_PROFILE_WAVES
  const unsigned long long t1_ = wall_clock64();
  if (lc.valid && lc.leg == 0) extra[lc.env * 6 + 5] = (float)(t1_ - t0_);
#endif
}

#if IRRL_LANES_PER_ROBOT == 16
// the fused step + policy kernel and the four persistent rollout kernels (env_rollout_kernels.hpp) with the shipped solver settings compiled in;
// their run-time-solver twins (_rt_l16) are the same text in a translation unit of their own (IRRL_ROLLOUT_RT_UNIT, above)
#define IRRL_RK(name) name##_l16
#define IRRL_ROLLOUT_RULE IRRL_RULE_SHIPPED
#include "env_rollout_kernels.hpp"
#undef IRRL_RK
#undef IRRL_ROLLOUT_RULE
#endif

// `count` CONSECUTIVE env.step()s IN ONE LAUNCH (irrl_env_step_rows_persistent[_out]): step k takes action row (first_row + k) % n_rows of a table
// resident in HBM.  Robots never interact (VEC:273), so a wave simply walks its own robots through the `count` steps: no grid-wide
// boundary between steps -- a step costs a wave its own time instead of the slowest of the 1024 waves, and the launch boundaries are gone.
// Round 5: the robots' lane context STAYS IN REGISTERS from step to step (load_lane once in front of the loop, store_lane once behind it;
// lane_carry() between two steps hands the next step exactly the words a store + load would have: env_core.hpp) -- a step no longer starts
// behind a round trip of ~90 stores and ~90 loads per lane through the L2.  The body of a step is the step kernel's (step_compute, same
// order): states and outputs are bit-identical to `count` launches of the step kernel with the same RULE.  Pools without the meteorite only; the
// launcher falls back otherwise.
}  // extern "C"
template <int RULE>
__device__ __forceinline__ void irrl_steps_persistent_body(const EnvParams &P_, const EnvState &S_, const float *action_rows, int n_rows, int first_row, int count,
                                                           float *ob, float *reward, uint8_t *done, float *extra, int out_rows) {
  (void)P_; (void)S_;   // (IRRL_BIND_ARGS names the kernel's first two arguments in the kernarg segment; the by-value copies serve the A/B build only)
  IRRL_BIND_ARGS
  const int blk = irrl_xcd_block();
  const size_t row = (size_t)P.n_envs * 12;
  // out_rows != 0: the outputs are [count, N, .] tables and step k fills row k -- the trajectory `count` step() calls of the reference
  // would have returned (VEC:268-278, RaisimGymVecEnv.py:26-52); 0: [N, .] arrays every step overwrites (the last step's survive)
  const size_t orow = out_rows ? (size_t)P.n_envs : (size_t)0;
  const LaneCtx lc = irrl_lane_ctx(P, blk * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63u));
  irrl_plain::EnvLane L;
  irrl_plain::load_lane(P, S, lc.env, lc.leg, L, true);
  // the action row of step k + 1 is requested while step k runs (three words per lane): a step does not start behind that round trip either
  irrl_plain::ActionRegs act_next;
  {
    const float *a0 = action_rows + row * (size_t)(first_row % n_rows) + (size_t)lc.env * 12 + lc.leg * 3;
    act_next.a[0] = a0[0]; act_next.a[1] = a0[1]; act_next.a[2] = a0[2];
  }
  for (int k = 0; k < count; k++) {
    // the lane's robot made opaque once per iteration: the per-lane addresses of the action row and of the output rows are then computed
    // inside the loop (hoisted, they are dozens of 64-bit values that spill)
    int env_ = lc.env;
    asm volatile("" : "+v"(env_));
    if (k > 0) irrl_plain::lane_carry(L);
    const irrl_plain::ActionRegs act = act_next;
    {
      const int kn = (k + 1 < count) ? k + 1 : k;      // (behind the last step: that step's own row once more)
      const float *an = action_rows + row * (size_t)((first_row + kn) % n_rows) + (size_t)env_ * 12 + lc.leg * 3;
      act_next.a[0] = an[0]; act_next.a[1] = an[1]; act_next.a[2] = an[2];
    }
    irrl_plain::step_compute<RULE, irrl_plain::NoStepHook, irrl_plain::NoStepTail, irrl_plain::ActionRegs>(
        IRRL_PARAMS_REFRESH(P), L, env_, lc.leg, lc.valid, act, ob + orow * 35 * (size_t)k, reward + orow * (size_t)k, done + orow * (size_t)k, extra + orow * 6 * (size_t)k);
  }
  if (count > 0) irrl_store_lane_back(P, S, lc.env, lc.leg, lc.valid, L);
}
extern "C" {
// the multi-step kernel per step-kernel variant that has one (the launcher picks, irrl_env_abi.hip kStepsKernels): the shipped solver settings
// compiled in with the run-time terrain test (rough ground) or with flat ground compiled in too; _rt = the published rule with the solver
// settings, the substep count and the terrain flag read from EnvParams (the step kernel _md's body); _dir = the build's first per-contact rule
// likewise (the step kernel _dir's body).  Pools with the meteorite (namespace irrl) have none.
#define IRRL_STEPS_KERNEL(NAME, RULE)                                                                                                       \
  __global__ void IRRL_ENV_BOUNDS                                                                                                           \
  IRRL_K(NAME)(EnvParams P_, EnvState S_, const float *action_rows, int n_rows, int first_row, int count, float *ob, float *reward,         \
               uint8_t *done, float *extra, int out_rows) {                                                                                 \
    irrl_steps_persistent_body<RULE>(P_, S_, action_rows, n_rows, first_row, count, ob, reward, done, extra, out_rows);                     \
  }
IRRL_STEPS_KERNEL(irrl_steps_persistent_kernel, IRRL_RULE_SHIPPED)
IRRL_STEPS_KERNEL(irrl_steps_persistent_kernel_flat, IRRL_RULE_SHIPPED_FLAT)
IRRL_STEPS_KERNEL(irrl_steps_persistent_kernel_rt, 1)
IRRL_STEPS_KERNEL(irrl_steps_persistent_kernel_dir, 0)

__global__ void IRRL_ENV_BOUNDS IRRL_K(irrl_init_kernel)(EnvParams P_, EnvState S_) {
  IRRL_BIND_ARGS
  IRRL_LANE_PROLOGUE
  irrl::init_body(P, S, lc.env, lc.leg, lc.valid);
}

__global__ void IRRL_ENV_BOUNDS IRRL_K(irrl_reset_kernel)(EnvParams P_, EnvState S_, float *ob) {
  IRRL_BIND_ARGS
  IRRL_LANE_PROLOGUE
  irrl::reset_body(P, S, lc.env, lc.leg, lc.valid, ob);
}

__global__ void IRRL_ENV_BOUNDS IRRL_K(irrl_observe_kernel)(EnvParams P_, EnvState S_, float *ob) {
  IRRL_BIND_ARGS
  IRRL_LANE_PROLOGUE
  irrl::observe_body(P, S, lc.env, lc.leg, lc.valid, ob);
}

__global__ void IRRL_ENV_BOUNDS IRRL_K(irrl_probe_kernel)(EnvParams P_, EnvState S_, float *minv, float *nonlin) {
  IRRL_BIND_ARGS
  IRRL_LANE_PROLOGUE
  irrl::dynamics_probe_body(P, S, lc.env, lc.leg, lc.valid, minv, nonlin);
}

#if IRRL_LANES_PER_ROBOT == 16
// isTerminalState (ENV:1553-1578) on the stored state; one thread per robot (layout independent: emitted once)
__global__ void irrl_terminal_kernel(EnvParams P_, EnvState S_, uint8_t *done) {
  IRRL_BIND_ARGS
  int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= P.n_envs) return;
  float z = S.gc[e * 19 + 2], up = S.ob[e * 35 + 31];
  done[e] = (z < 0.15f || z > 0.65f || up < 0.5f) ? 1 : 0;
}
#endif

}  // extern "C"

#endif  // IRRL_ROLLOUT_RT_UNIT
