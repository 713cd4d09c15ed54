// env_rollout_kernels.hpp -- the 16-lane kernels that run the policy in the same launch as the env step: the fused step + policy kernel and the
// four persistent rollout kernels.  NO INCLUDE GUARD: env_kernels.hip includes this file once per solver form, inside extern "C", with
//   IRRL_RK(name)      the kernel's name (name##_l16: the shipped solver settings compiled in; name##_rt_l16: read from EnvParams at run time)
//   IRRL_ROLLOUT_RULE  the RULE argument of step_body / step_compute (env_core.hpp: IRRL_RULE_SHIPPED, or 1 = the published rule, run-time settings)
// The text is preprocessed, not templated: the shipped kernels are the token sequence they were when they stood in env_kernels.hip (several are
// held to their ISA, see the written-out lane contexts below), and their run-time twins are the same text with another RULE.

// ONE ROLLOUT STEP IN ONE LAUNCH: env.step of 16 robots (the workgroup's four waves, four robots each: the step kernel's body
// unchanged) and, behind a workgroup barrier, the LSTM policy's step on the observations those 16 robots just produced (one
// MFMA M-tile; policy_step.hpp with two virtual waves per wave).  Published contact rule only (the launcher falls back otherwise).  `action` is what the previous launch's policy part wrote
// for these robots (a.clipped), `ob` / `done` / `reward` are a.obs / a.dones / a.prev_reward: nothing a workgroup touches
// belongs to another workgroup, so the only synchronisation is the barrier.  Against two launches per step this removes a
// launch boundary and hides the layer-0 weight fetch -- and still MEASURES SLOWER (62.9 against 58.2 us per step at 4096 envs,
// tools/rollout_phases.py): the launch ends with its slowest workgroup, which pays the whole policy part behind its slowest
// robot, and four waves (three of them with two virtual waves of MFMA work each) take 18.5 us for what the stand-alone kernel's
// six waves do in 14.1.  Bit-identical results; an OPTION of irrl_lstm_rollout (fuse = 1), not the default.  (HID 48, ob 35.)
__global__ void IRRL_ENV_BOUNDS
IRRL_RK(irrl_step_policy_kernel)(EnvParams P_, EnvState S_, const float *action, float *ob, float *reward, uint8_t *done, float *extra, PolicyStepArgs a_) {
  IRRL_BIND_ARGS
  IRRL_BIND_POLICY_ARGS_N(a, a_, 5)
  __shared__ float hbuf[2][16 * 49];
  __shared__ float terms[16][17];
  __shared__ float head_w[48 * 17];
  __shared__ __attribute__((aligned(1024))) float lds_w[PolicyLdsImage<48>::FLOATS];   // 126 KiB: wh0 | wx0 of the actor and the critic stack
#ifdef IRRL_PROFILE_POLICY
  const unsigned long long pt0_ = wall_clock64();
#endif
  {
    IRRL_LANE_PROLOGUE_IDENTITY
    // the env part keeps no LDS and, between its prologue and its epilogue, issues no global load (flat ground): the layer-0
    // policy weights travel L2 -> LDS underneath the eight substeps
    irrl_plain::step_body<IRRL_ROLLOUT_RULE>(P, S, lc.env, lc.leg, lc.valid, action, ob, reward, done, extra, [&]() { policy_prefetch_lds<48, 256>(a, lds_w); });
  }
#ifdef IRRL_PROFILE_POLICY
  const unsigned long long pt1_ = wall_clock64();
#else
  const unsigned long long pt0_ = 0, pt1_ = 0;
#endif
  __syncthreads();   // the workgroup's stores of obs / dones / reward are complete and visible to its own loads, the LDS image has landed
  policy_step_body<48, 9, 2, 256, true>(a, (int)blockIdx.x * 16, hbuf, terms, head_w, lds_w, pt0_, pt1_);
}

// THE WHOLE ROLLOUT IN ONE LAUNCH (persistent): a workgroup owns 16 robots -- its four env waves, one MFMA M-tile of the policy --
// for all `steps` control steps: policy step k -> barrier -> env.step k -> barrier -> policy step k + 1 ...  Robots never interact
// (VEC:273) and the policy is per-robot, so NOTHING crosses workgroups: there is no grid-wide boundary between steps, a step costs
// its workgroup's own time instead of the slowest of 1024 waves (mean 35.8 us against 43.4 us for the step kernel at 4096 envs,
// tools/wave_spread.py), the 2 x steps launch boundaries are gone, and the layer-0 weights are fetched into LDS ONCE.  The code of a
// step is the fused kernel's above (same device functions, same order): obs / dones / states / clipped actions / rollout rows are
// bit-identical to the two-launch sequence.  Within a workgroup every global array is written and re-read by the same CU: the
// vector L1 is coherent at workgroup scope (non-tgsplit), the barriers' waits on the memory counters order the accesses.
__global__ void IRRL_ENV_BOUNDS
IRRL_RK(irrl_rollout_persistent_kernel)(EnvParams P_, EnvState S_, float *ob, float *reward, uint8_t *done, float *extra, PolicyStepArgs a_, int steps) {
  IRRL_BIND_ARGS
  IRRL_BIND_POLICY_ARGS(a, a_)
  __shared__ float hbuf[2][16 * 49];
  __shared__ float terms[16][17];
  __shared__ float head_w[48 * 17];
  __shared__ __attribute__((aligned(1024))) float lds_w[PolicyLdsImage<48>::FLOATS];   // 126 KiB: wh0 | wx0 of the actor and the critic stack
  policy_prefetch_lds<48, 256>(a, lds_w);
  const PolicyStepBase base(a);
  __syncthreads();   // the LDS image has landed
#ifdef IRRL_PROFILE_PERSIST   /* diagnostic build (tools/persistent_phases.py): where a step goes, per wave, summed over the steps */
  unsigned long long ph_[4] = {0, 0, 0, 0}, pts_ = wall_clock64();
#define IRRL_PP_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long n_ = wall_clock64(); ph_[i] += n_ - pts_; pts_ = n_; __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define IRRL_PP_STAMP(i) do { } while (0)
#endif
  for (int k = 0; k < steps; k++) {
    // threadIdx.x made opaque once per iteration: every per-lane address below is then computed inside the loop (left to the
    // optimizer, the loop-invariant addresses of both parts -- hundreds of 64-bit values -- are hoisted and spilled)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const PolicyStepArgs ak = base.at(a, k);
    policy_step_body<48, 9, 2, 256, true>(ak, (int)blockIdx.x * 16, hbuf, terms, head_w, lds_w, 0, 0, tid);
    IRRL_PP_STAMP(0);   // policy step
    __syncthreads();   // this workgroup's clipped actions (and the rollout rows) are stored and visible to its own loads
    IRRL_PP_STAMP(1);   // barrier behind the policy step
    {
      const LaneCtx lc = irrl_lane_ctx(P, (int)blockIdx.x * 4 + (tid >> 6), tid & 63);
      irrl_plain::step_body<IRRL_ROLLOUT_RULE>(IRRL_PARAMS_REFRESH(P), IRRL_PARAMS_REFRESH(S), lc.env, lc.leg, lc.valid, (const float *)ak.clipped, ob, reward, done, extra);
    }
    IRRL_PP_STAMP(2);   // env step of this wave's four robots
    __syncthreads();   // obs / dones / reward of step k are stored and visible: the next policy step reads them
    IRRL_PP_STAMP(3);   // barrier behind the env step: waiting for the workgroup's slowest wave
  }
#ifdef IRRL_PROFILE_PERSIST
  if ((threadIdx.x & 63u) == 0u) {
    const int wv = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (wv * 4 < P.n_envs) for (int i = 0; i < 4; i++) extra[(size_t)wv * 4 * 6 + i] = (float)ph_[i];
  }
#endif
}

// THE LSTM ROLLOUT WITH THE CRITIC OFF THE PER-STEP PATH (round 5; irrl_lstm_rollout fuse = 3).  The value V(s_t) is a function of the
// observation history only -- nothing in the rollout depends on it until GAE -- so the per-step part runs the ACTOR stack alone and the
// caller evaluates the critic stack over the recorded [T, N, 35] observations afterwards with the update's sequence kernels (two launches
// for the whole rollout; ppo2.Runner).  What that buys per step: half the policy part's MFMAs and cells, and -- the LDS that held the critic's
// layer-0 operands now holds the actor's layer-1 operands -- NO weight fetched from L2 inside the step loop; the head weights are staged
// once.  Same device functions and per-element arithmetic as the full kernel above: actions, clipped actions, neglogp, observations,
// rewards, dones and the actor's LSTM state are bit-identical to every other rollout mode; `value` / `mb_values` are not written.
__global__ void IRRL_ENV_BOUNDS
IRRL_RK(irrl_rollout_persistent_actor_kernel)(EnvParams P_, EnvState S_, float *ob, float *reward, uint8_t *done, float *extra, PolicyStepArgs a_, int steps) {
  IRRL_BIND_ARGS
  IRRL_BIND_POLICY_ARGS(a, a_)
  __shared__ float hbuf[2][16 * 49];
  __shared__ float terms[16][17];
  __shared__ float head_w[48 * 17];
  __shared__ __attribute__((aligned(1024))) float lds_w[PolicyLdsImage<48>::FLOATS];   // wh0 | wx0 | wh1 | wx1 of the ACTOR stack
  policy_prefetch_lds_actor<48, 256>(a, lds_w);
  for (int i = (int)threadIdx.x; i < 48 * a.act_dim; i += 256) head_w[i] = a.pi_w[i];
  const PolicyStepBase base(a);
  // the env part's lane context stays in registers across the steps (irrl_steps_persistent_kernel below): with one virtual wave per wave the
  // policy part leaves room for it (379 registers, no scratch beyond the reset branch's).  (irrl_lane_ctx() written out: called here, it costs
  // this kernel a different register assignment from its first instructions on -- 212 of 17 981 lines -- and the kernel is held to its ISA.)
  const int lane0_ = (int)(threadIdx.x & 63u);
  int env0_ = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * 4 + (lane0_ >> 4);
  const int leg0_ = (lane0_ >> 2) & 3;
  const bool valid0_ = (env0_ < P.n_envs) && ((lane0_ & 3) == 0);
  if (env0_ >= P.n_envs) env0_ = P.n_envs - 1;
#ifndef IRRL_ACTOR_NO_CARRY      /* A/B switch of tools/build_variants.py */
  irrl_plain::EnvLane L;
  irrl_plain::load_lane(P, S, env0_, leg0_, L, true);
#endif
  __syncthreads();   // the LDS image and the head weights have landed
  for (int k = 0; k < steps; k++) {
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));     // (see irrl_rollout_persistent_kernel_l16: keeps the per-lane addresses inside the loop)
    const PolicyStepArgs ak = base.at(a, k);
    policy_step_body<48, 9, 1, 256, true, true>(ak, (int)blockIdx.x * 16, hbuf, terms, head_w, lds_w, 0, 0, tid);
    __syncthreads();   // this workgroup's clipped actions (and the rollout rows) are stored and visible to its own loads
    {
      int env_ = env0_;
      asm volatile("" : "+v"(env_));
#ifndef IRRL_ACTOR_NO_CARRY
      if (k > 0) irrl_plain::lane_carry(L);
      irrl_plain::step_compute<IRRL_ROLLOUT_RULE>(IRRL_PARAMS_REFRESH(P), L, env_, leg0_, valid0_, irrl_plain::ActionRow{(const float *)ak.clipped}, ob, reward, done, extra);
#else
      irrl_plain::step_body<IRRL_ROLLOUT_RULE>(IRRL_PARAMS_REFRESH(P), IRRL_PARAMS_REFRESH(S), env_, leg0_, valid0_, (const float *)ak.clipped, ob, reward, done, extra);
#endif
    }
    __syncthreads();   // obs / dones / reward of step k are stored and visible: the next policy step reads them
  }
#ifndef IRRL_ACTOR_NO_CARRY
  if (steps > 0) irrl_store_lane_back(P, S, env0_, leg0_, valid0_, L);
#endif
}

// THE ACTOR-ONLY ROLLOUT WITH THE POLICY AS EACH WAVE'S OWN WORK (round 5, second half; irrl_lstm_rollout fuse = 3, the default form of it).
// The kernel above still runs the actor for a workgroup's 16 robots on 16-row MFMA tiles: three barriers per step and, in every step, the
// wait for the slowest of the workgroup's four env waves.  Here a wave runs the actor stack for ITS four robots (lstm_actor_wave_body,
// policy_step.hpp: v_mfma_f32_4x4x1, operands out of a transposed LDS image), keeps h of both layers in its LDS scratch and c in registers for
// the whole rollout, and hands observations / reward / done flag / clipped actions between its env step and its policy step through that
// scratch next to the stores to memory -- no workgroup barrier and no load behind a store inside the step loop.  Actions, neglogp,
// observations, rewards, dones and the actor's final LSTM state are bit-identical to every other rollout mode.
__global__ void IRRL_ENV_BOUNDS
IRRL_RK(irrl_rollout_persistent_actor_wave_kernel)(EnvParams P_, EnvState S_, float *ob, float *reward, uint8_t *done, float *extra, PolicyStepArgs a_, int steps) {
  IRRL_BIND_ARGS
  IRRL_BIND_POLICY_ARGS(a, a_)
  constexpr int HID = 48, NG = HID / 16, SD = 8 * HID;
  typedef LstmWaveLds<HID> LAY;
  __shared__ __attribute__((aligned(16))) float wsl[4][LAY::FLOATS];
  __shared__ float head_w[HID * 16];
  __shared__ __attribute__((aligned(16))) float lds_w[LstmWaveImage<HID>::FLOATS];      // the ACTOR's operands, [gate column][K] (policy_step.hpp)
  lstm_wave_image_stage<HID, 256>(a, lds_w);
  for (int i = (int)threadIdx.x; i < HID * a.act_dim; i += 256) head_w[i] = a.pi_w[i];
  // (PolicyStepBase and irrl_lane_ctx() written out, here and in the step loop: with either of them this kernel gets another schedule and
  // register assignment -- same instruction count, thousands of lines moved -- and the kernel is held to its ISA)
  const float *noise0 = a.noise;
  const long long row0 = a.row, rng0 = a.rng_step;
  const size_t noise_stride = (size_t)a.N * (size_t)a.act_dim;
  const int lane0_ = (int)(threadIdx.x & 63u);
  const int wave_ = (int)(threadIdx.x >> 6);
  const int e4_ = ((int)blockIdx.x * 4 + wave_) * 4;            // the wave's first robot
  const int rl_ = lane0_ >> 4;                                   // the robot this lane integrates (env part)
  int env0_ = e4_ + rl_;
  const int leg0_ = (lane0_ >> 2) & 3;
  const bool valid0_ = (env0_ < P.n_envs) && ((lane0_ & 3) == 0);
  if (env0_ >= P.n_envs) env0_ = P.n_envs - 1;
  irrl_plain::EnvLane L;
  irrl_plain::load_lane(P, S, env0_, leg0_, L, true);
  float *ws = wsl[wave_];
  // policy part: this lane's robot is l & 3, its unit inside a column group l >> 2
  const int pr_ = lane0_ & 3, pq_ = lane0_ >> 2;
  const bool pok_ = e4_ + pr_ < a.N;
  const int pe_ = pok_ ? e4_ + pr_ : a.N - 1;
  float cst[2][NG], bias[2][NG];
#pragma unroll
  for (int G = 0; G < NG; G++) {
    cst[0][G] = a.states_in[(size_t)pe_ * SD + 16 * G + pq_];
    cst[1][G] = a.states_in[(size_t)pe_ * SD + 2 * HID + 16 * G + pq_];
    bias[0][G] = a.w[2][64 * G + lane0_];
    bias[1][G] = a.w[5][64 * G + lane0_];
  }
  {   // the state of things in front of step 0, from memory: observations, done flags, the last reward, h of both layers
    const int n = ((a.N - e4_ < 4) ? a.N - e4_ : 4);
    for (int i = lane0_; i < 4 * 35; i += 64) ws[LAY::X + i] = (i < n * 35) ? a.obs[(size_t)e4_ * 35 + i] : 0.0f;
    for (int i = lane0_; i < 4 * HID; i += 64) {
      const int r = i / HID, k = i - r * HID;
      const int e = (e4_ + r < a.N) ? e4_ + r : a.N - 1;
      ws[LAY::H0 + i] = a.states_in[(size_t)e * SD + HID + k];
      ws[LAY::H1 + i] = a.states_in[(size_t)e * SD + 3 * HID + k];
    }
    if (lane0_ < 4) {
      const int e = (e4_ + lane0_ < a.N) ? e4_ + lane0_ : a.N - 1;
      ws[LAY::DON + lane0_] = a.dones[e] ? 1.0f : 0.0f;
      ws[LAY::REW + lane0_] = a.prev_reward ? a.prev_reward[e] : 0.0f;
    }
  }
  __syncthreads();   // the LDS image and the head weights have landed
  for (int k = 0; k < steps; k++) {
    int lane = lane0_;
    asm volatile("" : "+v"(lane));
    PolicyStepArgs ak = IRRL_PARAMS_REFRESH(a);
    ak.row = row0 + k; ak.rng_step = rng0 + k;
    ak.noise = noise0 ? noise0 + (size_t)k * noise_stride : nullptr;
    lstm_actor_wave_body<HID>(ak, e4_, ws, lds_w, head_w, lane, cst, bias);
    PS_WAVE_SYNC();    // this wave's clipped actions are in its scratch
    {
      int env_ = env0_;
      asm volatile("" : "+v"(env_));
      if (k > 0) irrl_plain::lane_carry(L);
      irrl_plain::ActionRegs act;
#pragma unroll
      for (int j = 0; j < 3; j++) act.a[j] = ws[LAY::ACT + rl_ * 12 + leg0_ * 3 + j];
      irrl_plain::step_compute<IRRL_ROLLOUT_RULE, irrl_plain::NoStepHook>(
          IRRL_PARAMS_REFRESH(P), L, env_, leg0_, valid0_, act, ob, reward, done, extra, irrl_plain::NoStepHook(),
          [&](const irrl_plain::EnvLane &Lf, float rew, bool dn) {
            irrl_plain::observe_write(P, rl_, leg0_, valid0_, Lf, ws + LAY::X);
            if (valid0_ && leg0_ == 0) { ws[LAY::REW + rl_] = rew; ws[LAY::DON + rl_] = dn ? 1.0f : 0.0f; }
          });
    }
    PS_WAVE_SYNC();    // observations / done flags / rewards of step k are in the scratch
  }
  if (steps > 0) {
    irrl_store_lane_back(P, S, env0_, leg0_, valid0_, L);
    if (pok_) {      // the actor's LSTM state behind the last step (the critic's half is the caller's: ppo2.Runner._critic_pass)
#pragma unroll
      for (int G = 0; G < NG; G++) {
        const int u = 16 * G + pq_;
        a.states_out[(size_t)pe_ * SD + u] = cst[0][G];
        a.states_out[(size_t)pe_ * SD + HID + u] = ws[LAY::H0 + pr_ * HID + u];
        a.states_out[(size_t)pe_ * SD + 2 * HID + u] = cst[1][G];
        a.states_out[(size_t)pe_ * SD + 3 * HID + u] = ws[LAY::H1 + pr_ * HID + u];
      }
    }
  }
}

// THE SAME FOR MlpPolicy (BASELINE config 2's learner): the whole rollout in one launch.  The policy's 52 KB of weights and biases are copied
// to LDS ONCE (transposed: mlp_policy_stage_lds); a step of the policy part is then two MFMA chains on LDS operands + the heads (a few us
// against 8.7 us for the stand-alone launch, whose life is launch + weight fetch), and a step costs a WAVE its own time instead of the slowest
// of the 1024 env waves: since the second half of round 5 the policy of a wave's four robots is that wave's own work (see inside).
// Same device functions, same order: the buffers are bit-identical to the two-launch sequence.
__global__ void IRRL_ENV_BOUNDS
IRRL_RK(irrl_rollout_persistent_mlp_kernel)(EnvParams P_, EnvState S_, float *ob, float *reward, uint8_t *done, float *extra, PolicyStepArgs a_, int steps) {
  IRRL_BIND_ARGS
  IRRL_BIND_POLICY_ARGS(a, a_)
  typedef MlpWaveLds<64> LAY;
  __shared__ __attribute__((aligned(16))) float wsl[4][LAY::FLOATS];      // per wave: its four robots' scratch (policy_step.hpp)
  __shared__ float head_w[64 * 17];
  __shared__ __attribute__((aligned(16))) float wl[MlpLdsImage<64>::FLOATS];
  mlp_policy_stage_lds<64>(a, wl, head_w, (int)threadIdx.x, 256);
  const PolicyStepBase base(a);
  // the env part's lane context stays in registers across the steps (round 5; irrl_steps_persistent_kernel below): this policy's step needs
  // few registers (its weights and activations live in LDS), so the context survives it without spilling
  const int lane0_ = (int)(threadIdx.x & 63u);
  const int wave_ = (int)(threadIdx.x >> 6);
  const int e4_ = ((int)blockIdx.x * 4 + wave_) * 4;            // the wave's first robot
  const LaneCtx lc = irrl_lane_ctx(P, (int)blockIdx.x * 4 + wave_, lane0_);
  irrl_plain::EnvLane L;
  irrl_plain::load_lane(P, S, lc.env, lc.leg, L, true);
  // Round 5: the policy of a wave's four robots is that wave's own work (mlp_policy_wave_body): no workgroup barrier in the step loop, no wait
  // for the slowest of the four env waves in every step -- and what a wave hands from its env step to its policy step and back (observations,
  // reward, done flag; clipped actions) goes through its LDS scratch next to the stores to memory, so no load inside the loop waits for a store.
  float *ws = wsl[wave_];
  {   // the state of things in front of step 0, from memory: observations, done flags, the last reward
    const int n = ((a.N - e4_ < 4) ? a.N - e4_ : 4);
    for (int i = lane0_; i < 4 * 35; i += 64) ws[LAY::X + i] = (i < n * 35) ? a.obs[(size_t)e4_ * 35 + i] : 0.0f;
    if (lane0_ < 4) {
      const int e = (e4_ + lane0_ < a.N) ? e4_ + lane0_ : a.N - 1;
      ws[LAY::DON + lane0_] = a.dones[e] ? 1.0f : 0.0f;
      ws[LAY::REW + lane0_] = a.prev_reward ? a.prev_reward[e] : 0.0f;
    }
  }
  __syncthreads();
  for (int k = 0; k < steps; k++) {
    int lane = lane0_;
    asm volatile("" : "+v"(lane));     // (see irrl_rollout_persistent_kernel_l16: keeps the per-lane addresses inside the loop)
    const PolicyStepArgs ak = base.at(a, k);
    mlp_policy_wave_body<64, true, true>(ak, e4_, ws, wl, head_w, lane);
    PS_WAVE_SYNC();    // this wave's clipped actions are in its scratch
    {
      int env_ = lc.env;
      asm volatile("" : "+v"(env_));
      if (k > 0) irrl_plain::lane_carry(L);
      irrl_plain::ActionRegs act;
#pragma unroll
      for (int j = 0; j < 3; j++) act.a[j] = ws[LAY::ACT + lc.rw * 12 + lc.leg * 3 + j];
      irrl_plain::step_compute<IRRL_ROLLOUT_RULE, irrl_plain::NoStepHook>(
          IRRL_PARAMS_REFRESH(P), L, env_, lc.leg, lc.valid, act, ob, reward, done, extra, irrl_plain::NoStepHook(),
          [&](const irrl_plain::EnvLane &Lf, float rew, bool dn) {
            // (inside the epilogue's sub-lane-0 region) the scaled observation row, the reward and the done flag once more, into the scratch
            irrl_plain::observe_write(P, lc.rw, lc.leg, lc.valid, Lf, ws + LAY::X);
            if (lc.valid && lc.leg == 0) { ws[LAY::REW + lc.rw] = rew; ws[LAY::DON + lc.rw] = dn ? 1.0f : 0.0f; }
          });
    }
    PS_WAVE_SYNC();    // observations / done flags / rewards of step k are in the scratch: the wave's next policy step reads them
  }
  if (steps > 0) irrl_store_lane_back(P, S, lc.env, lc.leg, lc.valid, L);
}
