// eval_scenario_main.cpp -- the per-element functions of the device evaluation loop WITH A SCENARIO (csrc/eval_elements.hpp: command schedule,
// heading hold, statistics buckets) run on the HOST over a recorded sequence, in the order the five-launch form runs them:
// tests/test_eval_scenario_host.py compiles this file with g++ and the address / undefined-behaviour sanitizers, hands it a case file and compares
// what it writes with the numpy twins.  No HIP, no Python loading.  The twin of eval_elements_main.cpp.
//
//   eval_scenario_main <case file> <result file>
// case file:   int32 N, D, T, S, cmd_every, B, stat_every, t0 | f32 a_cmd, a_vel, a_act, mean[3], std[3], windup, heading_dt | int32 delay[N] |
//              f32 cmd_target[N][3] | f32 cmd_table[S][N][3] | f32 heading_ref[N], heading_kp[N], heading_ki[N] | f32 ob_reset[N][35] |
//              f32 q_reset[N][4] (the base quaternion in front of step 0) | f32 raw[T][N][35] (the env's observation after step t) | u8 done[T][N] |
//              f32 action[T][N][12] | f32 body[T][N][13] (after step t: its quaternion is what the heading hold of step t + 1 reads)
// result file: f32 cond[T][N][35] | f32 applied[T][N][12] | f64 stats[B][IRRL_EVAL_STAT_COUNT][N] | f32 cmd[N][3] | f32 vel_his[N][35] |
//              f32 I_cond[T][N] (the integrator behind the conditioning of step t) | f32 I_end[T][N] (behind the step's epilogue) |
//              int32 row[T] (the command row of step t) | int32 bucket[T]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eval_elements.hpp"

template <class T>
static void rd(FILE *f, T *p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "case file too short\n"); exit(2); }
}
template <class T>
static void wr(FILE *f, const T *p, size_t n) {
  if (fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); }
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[8];
  rd(f, hdr, 8);
  const int N = hdr[0], D = hdr[1], T = hdr[2], S = hdr[3], B = hdr[5];
  float sc[11];
  rd(f, sc, 11);
  std::vector<int> delay(N);
  std::vector<float> target((size_t)N * 3), table((size_t)S * N * 3), href(N), hkp(N), hki(N), ob_reset((size_t)N * 35), q_reset((size_t)N * 4),
      raw((size_t)T * N * 35), action((size_t)T * N * 12), body((size_t)T * N * 13);
  std::vector<uint8_t> done((size_t)T * N);
  rd(f, delay.data(), delay.size()); rd(f, target.data(), target.size()); rd(f, table.data(), table.size());
  rd(f, href.data(), href.size()); rd(f, hkp.data(), hkp.size()); rd(f, hki.data(), hki.size());
  rd(f, ob_reset.data(), ob_reset.size()); rd(f, q_reset.data(), q_reset.size()); rd(f, raw.data(), raw.size());
  rd(f, done.data(), done.size()); rd(f, action.data(), action.size()); rd(f, body.data(), body.size());
  fclose(f);

  // a fresh evaluation: every plane of the ring = the reset observation, everything else zero
  const size_t plane = (size_t)N * 35;
  std::vector<float> ring((size_t)D * plane), cmd((size_t)N * 3, 0.0f), vel_his(plane, 0.0f), act_his((size_t)N * 12, 0.0f), integ(N, 0.0f);
  for (int d = 0; d < D; d++)
    for (size_t i = 0; i < plane; i++) ring[(size_t)d * plane + i] = ob_reset[i];
  std::vector<double> stats((size_t)B * IRRL_EVAL_STAT_COUNT * N, 0.0);
  std::vector<float> cond((size_t)T * plane), applied((size_t)T * N * 12), i_cond((size_t)T * N), i_end((size_t)T * N);
  std::vector<int> rows(T), buckets(T);
  EvalArgs a = EvalArgs();
  a.N = N; a.D = D;
  a.a_cmd = sc[0]; a.a_vel = sc[1]; a.a_act = sc[2];
  a.mean0 = sc[3]; a.mean1 = sc[4]; a.mean2 = sc[5]; a.std0 = sc[6]; a.std1 = sc[7]; a.std2 = sc[8];
  a.t0 = hdr[7];
  a.cmd_rows = S; a.cmd_every = hdr[4]; a.cmd_table = table.data();
  a.stat_buckets = B; a.stat_every = hdr[6];
  a.heading_ref = href.data(); a.heading_kp = hkp.data(); a.heading_ki = hki.data(); a.heading_int = integ.data();
  a.heading_windup = sc[9]; a.heading_dt = sc[10];
  for (int t = 0; t < T; t++) {
    a.t = t;
    const long long tau = irrl_eval_tau(a, a.t);
    const int row = irrl_eval_cmd_row(a, tau), bucket = irrl_eval_stat_bucket(a, tau);
    rows[t] = row; buckets[t] = bucket;
    const float *obs = t == 0 ? ob_reset.data() : &raw[(size_t)(t - 1) * plane];
    for (int e = 0; e < N; e++) {
      for (int j = 0; j < 35; j++) {
        const size_t i = (size_t)e * 35 + j;
        float o = irrl_eval_condition_element(a, t % D, j, obs[i], &ring[i], plane, delay[e], &vel_his[i], j < 3 ? &cmd[(size_t)e * 3 + j] : nullptr,
                                              j < 3 ? &a.cmd_table[((size_t)row * N + e) * 3 + j] : nullptr);
        if (j == 2 && irrl_eval_heading_on(hkp[e], hki[e])) {
          const float *q = t == 0 ? &q_reset[(size_t)e * 4] : &body[((size_t)(t - 1) * N + e) * 13 + 3];
          o = irrl_eval_heading_element(a, href[e], hkp[e], hki[e], q[0], q[1], q[2], q[3], &integ[e]);
        }
        cond[(size_t)t * plane + i] = o;
      }
      i_cond[(size_t)t * N + e] = integ[e];
    }
    for (size_t i = 0; i < (size_t)N * 12; i++) applied[(size_t)t * N * 12 + i] = irrl_eval_action_element(a.a_act, action[(size_t)t * N * 12 + i], &act_his[i]);
    for (int e = 0; e < N; e++) {
      const float *b = &body[((size_t)t * N + e) * 13];
      const bool dn = done[(size_t)t * N + e] != 0;
      irrl_eval_heading_epilogue(dn, &integ[e]);
      irrl_eval_env_epilogue(dn, &cmd[(size_t)e * 3], &stats[(size_t)bucket * IRRL_EVAL_STAT_COUNT * N + e], (size_t)N, b[2], b[3], b[4], b[5], b[6], b[7], b[8], b[9],
                             b[10], b[11], b[12]);
      i_end[(size_t)t * N + e] = integ[e];
    }
  }
  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  wr(f, cond.data(), cond.size()); wr(f, applied.data(), applied.size()); wr(f, stats.data(), stats.size()); wr(f, cmd.data(), cmd.size());
  wr(f, vel_his.data(), vel_his.size()); wr(f, i_cond.data(), i_cond.size()); wr(f, i_end.data(), i_end.size()); wr(f, rows.data(), rows.size());
  wr(f, buckets.data(), buckets.size());
  fclose(f);
  return 0;
}
