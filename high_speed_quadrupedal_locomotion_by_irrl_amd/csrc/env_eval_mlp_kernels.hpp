// env_eval_mlp_kernels.hpp -- THE WHOLE POLICY EVALUATION IN ONE LAUNCH WITH MlpPolicy AS THE ACTOR (irrl_mlp_eval_measured_persistent): the closed
// loop of eval_rollout.hpp -- conditioning -> policy -> action filter -> env.step -> record -- for all `steps` control steps inside one persistent
// kernel: the structure of irrl_eval_persistent_kernel (env_eval_kernels.hpp) around the per-wave policy step of irrl_rollout_persistent_mlp_kernel
// (env_rollout_kernels.hpp).  NO INCLUDE GUARD: env_kernels.hip (its IRRL_EVAL_MLP_UNIT compilation, a translation unit of this kernel's own)
// includes this file once per solver form, inside extern "C", with IRRL_RK / IRRL_ROLLOUT_RULE as there.
//
// 256-thread workgroups of 16 robots; a WAVE owns robots e4 .. e4 + 3 for all steps: both networks' weights and biases go to LDS once, transposed
// (mlp_policy_stage_lds: 52 224 B), the head weights beside them, the env lane context stays in registers (load_lane once, lane_carry,
// irrl_store_lane_back once).  The policy has no recurrent state, so a wave's policy scratch (MlpWaveLds<64>: X | ACT | REW | DON | h1 | h2 |
// neglogp terms) holds nothing that outlives a step but X, the observation row the env step leaves for the next conditioning.  Beside it a wave
// keeps the evaluator's state of its robots in LDS for the whole launch: vel_his [4][35] | act_his [4][12] | cmd [4][3] (200 floats), the per-env
// parameters delay [4] | cmd_target [4][3], the f64 statistics [4][IRRL_EVAL_STAT_COUNT], the heading hold's scratch and the gait accumulators /
// staging / prev_contact -- read once in front of the loop, written back once behind it.  Only wave-level synchronisation inside the loop;
// nothing waits for another wave.  LDS: 52 224 (weight image) + 23 744 (four policy scratches) + 4 352 (heads) + about 11.5 KB of evaluator
// arrays, 92 KB of 160; one workgroup per CU under IRRL_ENV_BOUNDS.
//
// Per step k, element for element the arithmetic of the per-step form (eval_elements.hpp is the one text of it; the policy step is
// mlp_policy_wave_body, the body of the stand-alone mlp_policy_step_kernel), so every buffer the two forms share is BIT-IDENTICAL:
//   0. the scenario prologue (uniform for the whole grid): a new command row into EV_TG, the statistics / gait columns at a bucket boundary (the
//      old column back, the next one in), the kick of a step whose row fires on the lane context, the heading hold of the wave's robots,
//   1. conditioning of the wave's 4 x 35 elements: lane l owns elements l, l + 64, l + 128 for the whole launch.  The raw observation comes out
//      of the scratch X; the ring lives in the caller's buffer, and the lane that wrote a ring element is the only one that ever reads it.  The
//      conditioned row overwrites X (the ring holds the raw copy),
//   2. mlp_policy_wave_body<64, LDSW, XLDS, RAW_ACT> (deterministic: no noise, no rollout rows) on the LDS weight image: BOTH networks run, so the
//      work columns action | clipped | value | neglogp are written as the per-step form writes them; the scratch ACT gets the unclipped mean,
//   3. the [-1, 1] clip if the caller asked for it (the heads' own expression) and the action low-pass into ACT / act_his,
//   4. step_compute with the action out of ACT; its Tail hook sees the FINAL lane (post-reset on a `done`): observe_write into X, reward / done
//      into the scratch, the body / torque / reward / done recorders, cmd = 0 on done and the f64 statistics by the robot's lead lane (the
//      accumulators START from the caller's column), the quaternion for the next step's heading hold (the pool's gc in memory is stale inside the
//      loop),
//   5. the raw-observation recorder out of X, and the gait epilogue (staging by the legs' sub-lane 0, then lane r < 4 for robot r).
// The ring slot continues across calls (ev.slot = step0 % depth).  Idle rows of the pool's last wave shadow the last robot with their stores
// masked; a wave behind the pool's end computes the last robot's twin and stores nothing.  HID 64, ob 35, act 12.
__global__ void IRRL_ENV_BOUNDS
IRRL_RK(irrl_eval_mlp_persistent_kernel)(EnvParams P_, EnvState S_, float *ob, float *reward, uint8_t *done, float *extra, PolicyStepArgs a_, EvalArgs ev_) {
  IRRL_BIND_ARGS
  IRRL_BIND_POLICY_ARGS(a, a_)
  IRRL_BIND_EVAL_ARGS(ev, ev_)
  constexpr int HID = 64;
  constexpr int NS = IRRL_EVAL_STAT_COUNT;
  typedef MlpWaveLds<HID> LAY;
  // the evaluator's part of a wave's scratch (floats)
  constexpr int EV_VH = 0, EV_AH = 140, EV_CM = 188, EV_DL = 200, EV_TG = 204, EV_FLOATS = 216;
  // the scenario's heading hold, a wave's scratch of its own: base quaternion [4][4] | I [4] | ref [4] | kp [4] | ki [4] | the actor's element 2 [4]
  constexpr int EV_Q = 0, EV_HI = 16, EV_HR = 20, EV_HP = 24, EV_HK = 28, EV_HO = 32, HD_FLOATS = 36;
  __shared__ __attribute__((aligned(16))) float wsl[4][LAY::FLOATS];
  __shared__ __attribute__((aligned(16))) float evl[4][EV_FLOATS];
  __shared__ double stl[4][4 * NS];
  __shared__ float head_w[HID * 17];
  __shared__ float hdl[4][HD_FLOATS];
  // the gait measurements: accumulators [4][IRRL_EVAL_GAIT_COUNT] | the lead lane's staging tq [4][12], qd [4][12], lam_w [4][12] per robot | contact flags |
  // prev_contact
  constexpr int NGT = IRRL_EVAL_GAIT_COUNT, GS_FLOATS = 36;
  __shared__ double gtl[4][4 * NGT];
  __shared__ float gsl[4][4 * GS_FLOATS];
  __shared__ int gcl[4][4 * 4];
  __shared__ uint8_t pcl[4][4 * 4];
  __shared__ __attribute__((aligned(16))) float lds_w[MlpLdsImage<HID>::FLOATS];      // both networks' weights and biases, transposed (policy_step.hpp)
  mlp_policy_stage_lds<HID>(a, lds_w, head_w, (int)threadIdx.x, 256);
  const int steps = ev.steps;
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
  float *es = evl[wave_];
  float *hs = hdl[wave_];
  double *st = stl[wave_];
  // the wave's robots that exist: 4, fewer in the pool's last wave, none (<= 0) in a wave behind it
  const int nrob_ = (a.N - e4_ < 4) ? a.N - e4_ : 4;
  // the robot whose action this lane's env part applies: its own, or -- an idle row of the pool's last wave, which shadows the last robot with
  // its stores masked -- the last robot's, as the step kernel's clamped index reads it.  (The shadow must stay the last robot's exact twin: the
  // contact sweeps of a substep end for the whole wave at once, so a row that went its own way would change how many sweeps its neighbours get.)
  const int ra_ = rl_ < nrob_ ? rl_ : nrob_ > 0 ? nrob_ - 1 : 0;
  {   // the state of things in front of step 0, from memory: observations, done flags; the evaluator's state and parameters
    for (int i = lane0_; i < 4 * 35; i += 64) {
      const bool ok = i < nrob_ * 35;
      ws[LAY::X + i] = ok ? ev.obs[(size_t)e4_ * 35 + i] : 0.0f;
      es[EV_VH + i] = ok ? ev.vel_his[(size_t)e4_ * 35 + i] : 0.0f;
    }
    if (lane0_ < 4 * 12) {
      ws[LAY::ACT + lane0_] = 0.0f;
      es[EV_AH + lane0_] = (lane0_ < nrob_ * 12) ? ev.act_his[(size_t)e4_ * 12 + lane0_] : 0.0f;
    }
    if (lane0_ < 4 * 3) {
      const bool ok = lane0_ < nrob_ * 3;
      es[EV_CM + lane0_] = ok ? ev.cmd[(size_t)e4_ * 3 + lane0_] : 0.0f;
      es[EV_TG + lane0_] = ok ? ev.cmd_target[(size_t)e4_ * 3 + lane0_] : 0.0f;
    }
    if (lane0_ < 4) {
      const int e = (e4_ + lane0_ < a.N) ? e4_ + lane0_ : a.N - 1;
      ws[LAY::DON + lane0_] = a.dones[e] ? 1.0f : 0.0f;
      ws[LAY::REW + lane0_] = 0.0f;
      es[EV_DL + lane0_] = __int_as_float(ev.delay[e]);
    }
    if (ev.heading_kp) {   // the heading hold's state and parameters; the base quaternion as the pool holds it in front of step 0
      if (lane0_ < 16) {
        const int e = (e4_ + (lane0_ >> 2) < a.N) ? e4_ + (lane0_ >> 2) : a.N - 1;
        hs[EV_Q + lane0_] = ev.gc[(size_t)e * 19 + 3 + (lane0_ & 3)];
      }
      if (lane0_ < 4) {
        const int e = (e4_ + lane0_ < a.N) ? e4_ + lane0_ : a.N - 1;
        hs[EV_HI + lane0_] = ev.heading_int[e]; hs[EV_HR + lane0_] = ev.heading_ref[e];
        hs[EV_HP + lane0_] = ev.heading_kp[e]; hs[EV_HK + lane0_] = ev.heading_ki[e];
      }
    }
  }
  // the statistics bucket of step 0: the accumulators start from the caller's column of THAT bucket (a bucket boundary inside the loop writes
  // them back and loads the next bucket's, so the sequence of additions per bucket is the per-step form's)
  if (ev.stats) {
    const int bucket0 = irrl_eval_stat_bucket(ev, irrl_eval_tau(ev, ev.t));
    for (int i = lane0_; i < 4 * NS; i += 64) {
      const int r = i / NS, s = i - r * NS;
      st[i] = (r < nrob_) ? ev.stats[((size_t)bucket0 * NS + (size_t)s) * (size_t)a.N + (size_t)(e4_ + r)] : 0.0;
    }
  }
  // which parts of a scenario the call has, in ONE scalar register for the whole loop (see irrl_eval_persistent_kernel: a step without a scenario
  // tests this word and loads none of the scenario's kernel arguments; the scenario's blocks are marked unlikely)
  const int scn_ = __builtin_amdgcn_readfirstlane((ev.cmd_table ? 1 : 0) | (ev.stat_buckets > 1 ? 2 : 0) | (ev.heading_kp ? 4 : 0) | (ev.kick_table ? 8 : 0) |
                                                     ((ev.gait || ev.rec_gait || ev.prev_contact) ? 16 : 0));
  // the gait accumulators start from the caller's column of step 0's bucket, as `st` does; prev_contact comes in once
  if (__builtin_expect((scn_ & 16) != 0, 0)) {
    if (ev.gait) {
      const int bucket0 = irrl_eval_stat_bucket(ev, irrl_eval_tau(ev, ev.t));
      for (int i = lane0_; i < 4 * NGT; i += 64) {
        const int r = i / NGT, s = i - r * NGT;
        gtl[wave_][i] = (r < nrob_) ? ev.gait[((size_t)bucket0 * NGT + (size_t)s) * (size_t)a.N + (size_t)(e4_ + r)] : 0.0;
      }
    }
    if (lane0_ < 16) pcl[wave_][lane0_] = (ev.prev_contact && lane0_ < nrob_ * 4) ? ev.prev_contact[(size_t)e4_ * 4 + lane0_] : (uint8_t)0;
  }
  int slot_ = ev.slot;
  __syncthreads();   // the LDS image, the head weights and the wave's scratch have landed
  for (int k = 0; k < steps; k++) {
    int lane = lane0_;
    asm volatile("" : "+v"(lane));     // (see irrl_rollout_persistent_kernel_l16: keeps the per-lane addresses inside the loop)
    const EvalArgs &ek = IRRL_PARAMS_REFRESH(ev);
    const size_t rowk = (size_t)ek.row + (size_t)k;
    // ---- 0. the scenario, uniform for the whole grid: a new command row into EV_TG where the row index changes (and at k = 0); at a bucket
    //         boundary the accumulators go back to their bucket and the next bucket's columns come in; the heading hold of the wave's robots ----
    if (__builtin_expect((scn_ & 3) != 0, 0)) {
      const long long tk = ek.t + (long long)k;
      const long long tau = irrl_eval_tau(ek, tk), tau_before = irrl_eval_tau(ek, tk - 1);     // (tau_before is read for k > 0 only)
      if (scn_ & 1) {
        const int r = irrl_eval_cmd_row(ek, tau);
        if (k == 0 || r != irrl_eval_cmd_row(ek, tau_before)) {
          if (lane < nrob_ * 3) es[EV_TG + lane] = ek.cmd_table[((size_t)r * (size_t)ek.N + (size_t)e4_) * 3 + (size_t)lane];
          PS_WAVE_SYNC();
        }
      }
      if (k > 0 && ek.stats) {
        const int b = irrl_eval_stat_bucket(ek, tau), b_before = irrl_eval_stat_bucket(ek, tau_before);
        if (b != b_before) {
          for (int i = lane; i < nrob_ * NS; i += 64) {
            const int r = i / NS, s = i - r * NS;
            const size_t col = (size_t)s * (size_t)ek.N + (size_t)(e4_ + r);
            ek.stats[(size_t)b_before * NS * (size_t)ek.N + col] = st[i];
            st[i] = ek.stats[(size_t)b * NS * (size_t)ek.N + col];
          }
          PS_WAVE_SYNC();
        }
      }
      if (k > 0 && (scn_ & 18) == 18 && ek.gait) {     // the gait accumulators at the same boundary
        const int b = irrl_eval_stat_bucket(ek, tau), b_before = irrl_eval_stat_bucket(ek, tau_before);
        if (b != b_before) {
          double *gt = gtl[wave_];
          for (int i = lane; i < nrob_ * NGT; i += 64) {
            const int r = i / NGT, s = i - r * NGT;
            const size_t col = (size_t)s * (size_t)ek.N + (size_t)(e4_ + r);
            ek.gait[(size_t)b_before * NGT * (size_t)ek.N + col] = gt[i];
            gt[i] = ek.gait[(size_t)b * NGT * (size_t)ek.N + col];
          }
          PS_WAVE_SYNC();
        }
      }
    }
    // the kick of a step whose row fires (uniform for the whole grid), on the state the previous step or the reset left.  EVERY lane applies it
    // to its own copy of the robot's base state (see irrl_eval_persistent_kernel: the kick commutes with lane_carry's broadcast).  The heading
    // hold below reads the quaternion the Tail hook left in its scratch: pre-kick, as in the per-step form.  The row is the lane's clamped env's:
    // an idle row of the pool's last wave takes the last robot's kick and stays its exact twin.
    if (__builtin_expect((scn_ & 8) != 0, 0)) {
      const int r = irrl_eval_kick_row(ek, ek.t + (long long)k);
      if (r >= 0)
        irrl_eval_kick_apply(ek.kick_table + ((size_t)r * (size_t)ek.N + (size_t)env0_) * IRRL_EVAL_KICK_DIM, L.pos.z, L.qw, L.qx, L.qy, L.qz, L.vw.x, L.vw.y,
                             L.vw.z, L.ww.x, L.ww.y, L.ww.z);
    }
    if (__builtin_expect((scn_ & 4) != 0, 0)) {
      if (lane < nrob_) {
        const float kp = hs[EV_HP + lane], ki = hs[EV_HK + lane];
        if (irrl_eval_heading_on(kp, ki))
          hs[EV_HO + lane] = irrl_eval_heading_element(ek, hs[EV_HR + lane], kp, ki, hs[EV_Q + lane * 4], hs[EV_Q + lane * 4 + 1], hs[EV_Q + lane * 4 + 2],
                                                       hs[EV_Q + lane * 4 + 3], hs + EV_HI + lane);
      }
      PS_WAVE_SYNC();
    }
    // ---- 1. conditioning: this lane's elements lane, lane + 64, lane + 128 of the wave's [4][35] ----
    {
      const size_t plane = (size_t)ek.N * 35;
#pragma unroll
      for (int u = 0; u < 3; u++) {
        const int i = lane + 64 * u;
        if (i < nrob_ * 35) {
          const int r = i / 35, j = i - r * 35;
          const size_t gi = (size_t)e4_ * 35 + (size_t)i;
          float o = irrl_eval_condition_element(ek, slot_, j, ws[LAY::X + i], ek.ring + gi, plane, __float_as_int(es[EV_DL + r]), es + EV_VH + i,
                                                es + EV_CM + r * 3 + j, es + EV_TG + r * 3 + j);
          if (__builtin_expect((scn_ & 4) != 0, 0) && j == 2 && irrl_eval_heading_on(hs[EV_HP + r], hs[EV_HK + r])) o = hs[EV_HO + r];   // the heading hold's element 2
          ws[LAY::X + i] = o;
          ek.obs_cond[gi] = o;
          if (ek.rec_obs_cond) ek.rec_obs_cond[rowk * plane + gi] = o;
        }
      }
    }
    PS_WAVE_SYNC();    // the conditioned rows are in the scratch
    // ---- 2. MlpPolicy of the wave's four robots, both networks: action | clipped | value | neglogp go to the work array as the stand-alone step
    //         writes them ----
    {
      const PolicyStepArgs ak = IRRL_PARAMS_REFRESH(a);
      mlp_policy_wave_body<HID, true, true, true>(ak, e4_, ws, lds_w, head_w, lane);
    }
    PS_WAVE_SYNC();    // this wave's actions (the mean, before the clip) are in its scratch
    // ---- 3. clip and action low-pass: lane (robot, action) ----
    if (lane < nrob_ * 12) {
      const float act = ws[LAY::ACT + lane];
      const float x = ek.clip ? fminf(fmaxf(act, -1.0f), 1.0f) : act;
      const float y = irrl_eval_action_element(ek.a_act, x, es + EV_AH + lane);
      ws[LAY::ACT + lane] = y;
      const size_t gi = (size_t)e4_ * 12 + (size_t)lane;
      ek.applied[gi] = y;
      const size_t r = rowk * (size_t)ek.N * 12 + gi;
      if (ek.rec_act_clipped) ek.rec_act_clipped[r] = x;
      if (ek.rec_act_applied) ek.rec_act_applied[r] = y;
    }
    PS_WAVE_SYNC();    // the applied actions are in the scratch
    // ---- 4. env.step of the wave's four robots ----
    {
      int env_ = env0_;
      asm volatile("" : "+v"(env_));
      if (k > 0) irrl_plain::lane_carry(L);
      irrl_plain::ActionRegs act;
#pragma unroll
      for (int j = 0; j < 3; j++) act.a[j] = ws[LAY::ACT + ra_ * 12 + leg0_ * 3 + j];
      irrl_plain::step_compute<IRRL_ROLLOUT_RULE, irrl_plain::NoStepHook>(
          IRRL_PARAMS_REFRESH(P), L, env_, leg0_, valid0_, act, ob, reward, done, extra, irrl_plain::NoStepHook(),
          [&](const irrl_plain::EnvLane &Lf, float rew, bool dn) {
            // (inside the epilogue's sub-lane-0 region) the scaled observation row, the reward and the done flag once more, into the scratch
            irrl_plain::observe_write(P, rl_, leg0_, valid0_, Lf, ws + LAY::X);
            if (valid0_) {
              const size_t N = (size_t)ek.N, e = (size_t)env_;
              if (ek.rec_torque) {
                float *t = ek.rec_torque + rowk * N * 12 + e * 12 + leg0_ * 3;
                t[0] = Lf.tq[0]; t[1] = Lf.tq[1]; t[2] = Lf.tq[2];
              }
              if (leg0_ == 0) {
                ws[LAY::REW + rl_] = rew; ws[LAY::DON + rl_] = dn ? 1.0f : 0.0f;
                if (ek.rec_body) {     // base x y z, quaternion wxyz | world linear and angular velocity: the words store_lane leaves in the pool
                  float *b = ek.rec_body + rowk * N * 13 + e * 13;
                  b[0] = Lf.pos.x; b[1] = Lf.pos.y; b[2] = Lf.pos.z; b[3] = Lf.qw; b[4] = Lf.qx; b[5] = Lf.qy; b[6] = Lf.qz;
                  b[7] = Lf.vw.x; b[8] = Lf.vw.y; b[9] = Lf.vw.z; b[10] = Lf.ww.x; b[11] = Lf.ww.y; b[12] = Lf.ww.z;
                }
                if (ek.rec_reward) ek.rec_reward[rowk * N + e] = rew;
                if (ek.rec_done) ek.rec_done[rowk * N + e] = dn ? 1 : 0;
                irrl_eval_env_epilogue(dn, es + EV_CM + rl_ * 3, ek.stats ? st + rl_ * NS : nullptr, (size_t)1, Lf.pos.z, Lf.qw, Lf.qx, Lf.qy, Lf.qz, Lf.vw.x,
                                       Lf.vw.y, Lf.vw.z, Lf.ww.x, Lf.ww.y, Lf.ww.z);
                if (__builtin_expect((scn_ & 4) != 0, 0)) {   // the pool's gc in memory is stale inside the loop: the next step's heading hold reads the FINAL lane's quaternion here
                  float *q = hs + EV_Q + rl_ * 4;
                  q[0] = Lf.qw; q[1] = Lf.qx; q[2] = Lf.qy; q[3] = Lf.qz;
                  irrl_eval_heading_epilogue(dn, hs + EV_HI + rl_);
                }
              }
            }
          });
    }
    PS_WAVE_SYNC();    // observations / done flags / the reset commands of step k are in the scratch
    // ---- 5. the raw-observation recorder: the row the env step just left in X ----
    if (ek.rec_obs_raw) {
      const size_t plane = (size_t)ek.N * 35;
#pragma unroll
      for (int u = 0; u < 3; u++) {
        const int i = lane + 64 * u;
        if (i < nrob_ * 35) ek.rec_obs_raw[rowk * plane + (size_t)e4_ * 35 + (size_t)i] = ws[LAY::X + i];
      }
    }
    // ---- 5b. the gait measurements, one block behind the env step.  L is the FINAL lane context (the Tail hook's Lf, post-reset on a `done`):
    //          every leg's sub-lane 0 of a robot that exists leaves its three torques, rates and impulses and its contact flag in the wave's
    //          scratch, in the pool's order; then lane r < nrob_ owns robot r's column, prev_contact bytes and recorder row, and adds in the
    //          per-step kernel's index order (the done flag out of the scratch) ----
    if (__builtin_expect((scn_ & 16) != 0, 0)) {
      if (valid0_) {
        float *gs = gsl[wave_] + rl_ * GS_FLOATS;
#pragma unroll
        for (int j = 0; j < 3; j++) {
          gs[leg0_ * 3 + j] = L.tq[j]; gs[12 + leg0_ * 3 + j] = L.qd[j]; gs[24 + leg0_ * 3 + j] = L.lamw[j];
        }
        gcl[wave_][rl_ * 4 + leg0_] = L.in_contact;
      }
      PS_WAVE_SYNC();
      if (lane < nrob_) {
        const float *gs = gsl[wave_] + lane * GS_FLOATS;
        const int *gc = gcl[wave_] + lane * 4;
        if (ek.rec_gait)
          irrl_eval_gait_record(ek.rec_gait + (rowk * (size_t)ek.N + (size_t)(e4_ + lane)) * IRRL_EVAL_GAIT_REC_DIM, gs, gs + 12, gc, gs + 24, ek.inv_control_dt);
        irrl_eval_gait_epilogue(ws[LAY::DON + lane] != 0.0f, ek.gait ? gtl[wave_] + lane * NGT : nullptr, (size_t)1, ek.prev_contact ? pcl[wave_] + lane * 4 : nullptr,
                                gs, gs + 12, gc, gs + 24, ek.inv_control_dt);
      }
      PS_WAVE_SYNC();
    }
    slot_ = slot_ + 1 == ek.D ? 0 : slot_ + 1;
  }
  if (steps > 0) {
    irrl_store_lane_back(P, S, env0_, leg0_, valid0_, L);
    PS_WAVE_SYNC();
    // the evaluator's state behind the last step (obs / done were stored by the env step itself)
    for (int i = lane0_; i < nrob_ * 35; i += 64) ev.vel_his[(size_t)e4_ * 35 + i] = es[EV_VH + i];
    if (lane0_ < nrob_ * 12) ev.act_his[(size_t)e4_ * 12 + lane0_] = es[EV_AH + lane0_];
    if (lane0_ < nrob_ * 3) ev.cmd[(size_t)e4_ * 3 + lane0_] = es[EV_CM + lane0_];
    if (ev.heading_kp && lane0_ < nrob_) ev.heading_int[e4_ + lane0_] = hs[EV_HI + lane0_];
    if (ev.stats) {
      const int bucket1 = irrl_eval_stat_bucket(ev, irrl_eval_tau(ev, ev.t + (long long)(steps - 1)));     // the last step's bucket
      for (int i = lane0_; i < nrob_ * NS; i += 64) {
        const int r = i / NS, s = i - r * NS;
        ev.stats[((size_t)bucket1 * NS + (size_t)s) * (size_t)a.N + (size_t)(e4_ + r)] = st[i];
      }
    }
    if (__builtin_expect((scn_ & 16) != 0, 0)) {
      if (ev.gait) {
        const int bucket1 = irrl_eval_stat_bucket(ev, irrl_eval_tau(ev, ev.t + (long long)(steps - 1)));
        for (int i = lane0_; i < nrob_ * NGT; i += 64) {
          const int r = i / NGT, s = i - r * NGT;
          ev.gait[((size_t)bucket1 * NGT + (size_t)s) * (size_t)a.N + (size_t)(e4_ + r)] = gtl[wave_][i];
        }
      }
      if (ev.prev_contact && lane0_ < nrob_ * 4) ev.prev_contact[(size_t)e4_ * 4 + lane0_] = pcl[wave_][lane0_];
    }
  }
}
