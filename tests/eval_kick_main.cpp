// eval_kick_main.cpp -- the kick of the device evaluation loop (csrc/eval_elements.hpp: irrl_eval_kick_row, irrl_eval_kick_on, irrl_eval_kick_apply)
// run on the HOST: tests/test_eval_kick_host.py compiles this file with g++ and the address / undefined-behaviour sanitizers, hands it a case file
// and compares what it writes with the numpy twins (evaluate.apply_kick, evaluate.kick_row_index).  No HIP, no Python loading.  The twin of
// eval_scenario_main.cpp.
//
//   eval_kick_main <case file> <result file>
// case file:   int32 N, kick_rows, kick_every, t_lo, t_hi | int64 t0, kick_first |
//              f32 base[N][11] (z | quaternion w x y z | world linear velocity | world angular velocity: gc[2:7], gv[0:6]) | f32 kick[N][11]
// result file: f32 base_after[N][11] | int32 on[N] | int32 row[t_hi - t_lo] (the row that fires at t_lo <= t < t_hi, or -1)
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
  if (n == 0) return;     // (an empty vector's data() may be NULL)
  if (fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); }
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[5];
  long long sched[2];
  rd(f, hdr, 5);
  rd(f, sched, 2);
  const int N = hdr[0], t_lo = hdr[3], t_hi = hdr[4];
  if (N < 0 || t_hi < t_lo) { fprintf(stderr, "bad header\n"); return 2; }
  std::vector<float> base((size_t)N * IRRL_EVAL_KICK_DIM), kick((size_t)N * IRRL_EVAL_KICK_DIM);
  rd(f, base.data(), base.size());
  rd(f, kick.data(), kick.size());
  fclose(f);

  std::vector<int> on(N), rows((size_t)(t_hi - t_lo));
  for (int e = 0; e < N; e++) {
    float *b = &base[(size_t)e * IRRL_EVAL_KICK_DIM];
    const float *k = &kick[(size_t)e * IRRL_EVAL_KICK_DIM];
    on[e] = irrl_eval_kick_on(k) ? 1 : 0;
    irrl_eval_kick_apply(k, b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], b[9], b[10]);
  }
  EvalArgs a = EvalArgs();
  a.N = N;
  a.t0 = sched[0];
  a.kick_rows = hdr[1]; a.kick_every = hdr[2]; a.kick_first = sched[1]; a.kick_table = kick.data();
  for (int t = t_lo; t < t_hi; t++) rows[(size_t)(t - t_lo)] = irrl_eval_kick_row(a, (long long)t);

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  wr(f, base.data(), base.size()); wr(f, on.data(), on.size()); wr(f, rows.data(), rows.size());
  fclose(f);
  return 0;
}
