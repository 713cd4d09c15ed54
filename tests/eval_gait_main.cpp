// eval_gait_main.cpp -- the gait measurements of the device evaluation loop (csrc/eval_elements.hpp: irrl_eval_gait_epilogue, irrl_eval_gait_record,
// irrl_eval_stat_bucket) run on the HOST: tests/test_eval_gait_host.py compiles this file with g++ and the address / undefined-behaviour
// sanitizers, hands it a case file and compares what it writes with the numpy twin (evaluate.gait_rows_numpy).  No HIP, no Python loading.  The
// twin of eval_kick_main.cpp.
//
//   eval_gait_main <case file> <result file>
// case file:   int32 T, N, stat_buckets, stat_every | int64 t, t0 | f32 inv_control_dt |
//              f32 tq[T][N][12] | f32 qd[T][N][12] | int32 in_contact[T][N][4] | f32 lamw[T][N][4][3] | u8 done[T][N] | u8 prev_contact[N][4]
// result file: f64 gait[max(stat_buckets, 1)][IRRL_EVAL_GAIT_COUNT][N] | u8 prev_contact[N][4] | f32 rec_gait[T][N][32]
// The rows of step k go through the record kernel's statements: the recorder's row, then the epilogue on the env's column of the step's bucket.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eval_elements.hpp"

template <class T>
static void rd(FILE *f, T *p, size_t n) {
  if (n == 0) return;
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
  int hdr[4];
  long long when[2];
  float inv_dt;
  rd(f, hdr, 4);
  rd(f, when, 2);
  rd(f, &inv_dt, 1);
  const int T = hdr[0], N = hdr[1];
  if (T < 0 || N < 0) { fprintf(stderr, "bad header\n"); return 2; }
  const size_t TN = (size_t)T * (size_t)N;
  std::vector<float> tq(TN * 12), qd(TN * 12), lamw(TN * 12);
  std::vector<int> contact(TN * 4);
  std::vector<uint8_t> done(TN), prev((size_t)N * 4);
  rd(f, tq.data(), tq.size()); rd(f, qd.data(), qd.size()); rd(f, contact.data(), contact.size()); rd(f, lamw.data(), lamw.size());
  rd(f, done.data(), done.size()); rd(f, prev.data(), prev.size());
  fclose(f);

  EvalArgs a = EvalArgs();
  a.N = N;
  a.t0 = when[1];
  a.stat_buckets = hdr[2]; a.stat_every = hdr[3];
  const int B = hdr[2] < 1 ? 1 : hdr[2];
  std::vector<double> gait((size_t)B * IRRL_EVAL_GAIT_COUNT * (size_t)N, 0.0);
  std::vector<float> rec(TN * IRRL_EVAL_GAIT_REC_DIM);
  for (int k = 0; k < T; k++) {
    a.t = when[0] + k;
    const size_t bucket = (size_t)irrl_eval_stat_bucket(a, irrl_eval_tau(a, a.t)) * (size_t)IRRL_EVAL_GAIT_COUNT * (size_t)N;
    for (int e = 0; e < N; e++) {
      const size_t r = (size_t)k * (size_t)N + (size_t)e;
      irrl_eval_gait_record(&rec[r * IRRL_EVAL_GAIT_REC_DIM], &tq[r * 12], &qd[r * 12], &contact[r * 4], &lamw[r * 12], inv_dt);
      irrl_eval_gait_epilogue(done[r] != 0, &gait[bucket + (size_t)e], (size_t)N, &prev[(size_t)e * 4], &tq[r * 12], &qd[r * 12], &contact[r * 4], &lamw[r * 12],
                              inv_dt);
    }
  }

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  wr(f, gait.data(), gait.size()); wr(f, prev.data(), prev.size()); wr(f, rec.data(), rec.size());
  fclose(f);
  return 0;
}
