// eval_recurrence_main.cpp -- the per-pair arithmetic of the recurrence analysis (csrc/eval_elements.hpp: irrl_eval_recurrence_row, _state,
// _dist2, _level, _threshold, _spec_error, on top of irrl_eval_ensemble_features) run on the HOST from a plain serial O(T^2) loop in place of the
// kernel's diagonal and column walks: tests/test_eval_recurrence_host.py compiles this file with g++ and the address / undefined-behaviour
// sanitizers, hands it a case file and compares what it writes with the numpy twin (evaluate.recurrence_numpy).  No HIP, no Python loading.
// The twin of eval_ensemble_main.cpp.
//
//   eval_recurrence_main <case file> <result file>
// case file:   int32 rows, N, frame_first, frame_every, T | f64 lb[6] ub[6] eps | int32 steps radius theiler lmin vmin lags matrix_count
//              matrix_env[8] | f32 body[rows][N][13]
// result file: u8 q[N][T][T] | u32 counts[N][9] | u32 lag[N][lags] | u32 pairs in which (level < radius) != (d2 < threshold)
// A spec that irrl_eval_recurrence_spec_error refuses (or lags > T): the text on stderr, exit status 3, no result file.
#include <cmath>
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
  if (n == 0) return;
  if (fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "write failed\n"); exit(2); }
}

// a line of `run` points ends
static void close_line(uint32_t run, uint32_t least, uint32_t *points, uint32_t *lines, uint32_t *longest) {
  if (run == 0) return;
  if (run >= least) { *points += run; *lines += 1; }
  if (run > *longest) *longest = run;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[5];
  rd(f, hdr, 5);
  irrl_eval_recurrence_spec spec;
  rd(f, spec.lb, 6); rd(f, spec.ub, 6); rd(f, &spec.eps, 1);
  int ints[7];
  rd(f, ints, 7);
  spec.steps = ints[0]; spec.radius = ints[1]; spec.theiler = ints[2]; spec.lmin = ints[3]; spec.vmin = ints[4]; spec.lags = ints[5];
  spec.matrix_count = ints[6];
  rd(f, spec.matrix_env, 8);
  const int rows = hdr[0], N = hdr[1], frame_first = hdr[2], frame_every = hdr[3], T = hdr[4];
  if (rows < 0 || N < 1 || T < 0 || T > IRRL_EVAL_RECURRENCE_MAX_FRAMES || frame_first < 0 || frame_every < 1 ||
      (T > 0 && irrl_eval_recurrence_row(frame_first, frame_every, T - 1) >= rows)) { fprintf(stderr, "bad header\n"); return 2; }
  if (const char *bad = irrl_eval_recurrence_spec_error(spec)) { fprintf(stderr, "spec: %s\n", bad); return 3; }
  if (spec.lags > T) { fprintf(stderr, "spec: lags lies in 0 .. frames\n"); return 3; }
  std::vector<float> body((size_t)rows * (size_t)N * 13);
  rd(f, body.data(), body.size());
  fclose(f);

  const int W = spec.theiler > 1 ? spec.theiler : 1, lags = spec.lags;
  const double thr = irrl_eval_recurrence_threshold(spec.eps, spec.steps, spec.radius);
  const size_t TT = (size_t)T * (size_t)T;
  std::vector<uint8_t> q((size_t)N * TT, 0);
  std::vector<uint32_t> counts((size_t)N * IRRL_EVAL_RECURRENCE_COUNTS, 0), lag((size_t)N * (size_t)lags, 0);
  uint32_t disagree = 0;
  std::vector<double> u((size_t)T * 6);
  std::vector<uint8_t> kept((size_t)T);
  for (int e = 0; e < N; e++) {
    uint32_t *c = &counts[(size_t)e * IRRL_EVAL_RECURRENCE_COUNTS];
    uint8_t *qe = q.data() + (size_t)e * TT;
    for (int i = 0; i < T; i++) {
      const size_t row = (size_t)irrl_eval_recurrence_row(frame_first, frame_every, i);
      double x[6];
      irrl_eval_ensemble_features(&body[(row * (size_t)N + (size_t)e) * 13], x);
      kept[(size_t)i] = irrl_eval_recurrence_state(x, spec, &u[(size_t)i * 6], 1) ? 1 : 0;
      if (!kept[(size_t)i])
        for (int k = 0; k < 6; k++) u[(size_t)i * 6 + (size_t)k] = 0.0;
      c[0] += kept[(size_t)i];
    }
    // the levels of every ordered pair
    for (int i = 0; i < T; i++)
      for (int j = 0; j < T; j++) {
        int level = spec.steps;
        if (kept[(size_t)i] && kept[(size_t)j]) {
          const double d2 = irrl_eval_recurrence_dist2(&u[(size_t)i * 6], 1, &u[(size_t)j * 6], 1);
          level = irrl_eval_recurrence_level(d2, spec.eps, spec.steps);
          if ((level < spec.radius) != (d2 < thr)) disagree++;
        }
        qe[(size_t)i * (size_t)T + (size_t)j] = (uint8_t)level;
      }
    // diagonals tau = 0 .. T - 1 of the upper triangle
    for (int tau = 0; tau < T; tau++) {
      uint32_t run = 0, cnt = 0, points = 0, lines = 0, longest = 0;
      for (int i = 0; i + tau < T; i++) {
        if (qe[(size_t)i * (size_t)T + (size_t)(i + tau)] < spec.radius) { run++; cnt++; }
        else { close_line(run, (uint32_t)spec.lmin, &points, &lines, &longest); run = 0; }
      }
      close_line(run, (uint32_t)spec.lmin, &points, &lines, &longest);
      if (tau < lags) lag[(size_t)e * (size_t)lags + (size_t)tau] = cnt;
      if (tau >= W) { c[1] += cnt; c[2] += points; c[3] += lines; if (longest > c[4]) c[4] = longest; }
    }
    // columns of the full matrix without the band |i - j| < w
    for (int j = 0; j < T; j++) {
      uint32_t run = 0;
      for (int i = 0; i < T; i++) {
        const int gap = i > j ? i - j : j - i;
        if (gap >= W && qe[(size_t)i * (size_t)T + (size_t)j] < spec.radius) { run++; c[8]++; }
        else { close_line(run, (uint32_t)spec.vmin, &c[5], &c[6], &c[7]); run = 0; }
      }
      close_line(run, (uint32_t)spec.vmin, &c[5], &c[6], &c[7]);
    }
  }

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  wr(f, q.data(), q.size()); wr(f, counts.data(), counts.size()); wr(f, lag.data(), lag.size()); wr(f, &disagree, 1);
  fclose(f);
  return 0;
}
