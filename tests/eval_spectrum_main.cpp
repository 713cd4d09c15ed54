// eval_spectrum_main.cpp -- the spectrogram and the Welch spectrum (csrc/eval_elements.hpp: irrl_eval_spectrum_bins, _segments, _sample, _mean,
// _windowed, _add, _step, _gain, _power, _density, _work_per_env, _spec_error; irrl_eval_recurrence_row) run on the HOST from plain serial loops in
// the stated order -- per bin the samples ascending from +0.0, per robot the segments ascending from +0.0, per condition the robots ascending from
// +0.0: tests/test_eval_spectrum_host.py compiles this file with g++ and the address / undefined-behaviour sanitizers, hands it a case file and
// compares what it writes with the numpy twin (evaluate.spectrum_numpy).  No HIP, no Python loading.
//
//   eval_spectrum_main <case file> <result file>
//   eval_spectrum_main tables <nperseg> <window_kind> <alpha> <result file>       f64 window[nperseg] | f64 tw[nperseg][2]
// case file:   int32 rows, N, frame_first, frame_every, T, has_done, conditions | int32 x_dim, x_first, x_count, nperseg, hop, detrend, matrix_count,
//              matrix_env[8] | f64 fs, scale[64] | f64 window[nperseg] | f64 tw[nperseg][2] | f32 x[rows][N][x_dim] | u8 rec_done[rows][N] if has_done
// result file: i64 segments[C] | f64 psd_sum[C][cx][K] | f64 sxx[matrix_count][cx][S_max][K] | u64 irrl_eval_spectrum_work_per_env
// A spec that irrl_eval_spectrum_spec_error refuses: the text on stderr, exit status 3, no result file.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
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

static int tables(char **argv) {
  const int nperseg = atoi(argv[2]), kind = atoi(argv[3]);
  const double alpha = atof(argv[4]);
  std::vector<double> window((size_t)(nperseg > 0 ? nperseg : 0)), tw(2 * window.size());
  if (const char *bad = irrl_eval_spectrum_tables_error(nperseg, kind, alpha, window.data(), tw.data())) { fprintf(stderr, "tables: %s\n", bad); return 3; }
  irrl_eval_spectrum_tables_fill(nperseg, kind, alpha, window.data(), tw.data());
  FILE *f = fopen(argv[5], "wb");
  if (!f) { perror(argv[5]); return 2; }
  wr(f, window.data(), window.size());
  wr(f, tw.data(), tw.size());
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 6 && std::string(argv[1]) == "tables") return tables(argv);
  if (argc != 3) { fprintf(stderr, "usage: %s <case file> <result file> | tables <nperseg> <window_kind> <alpha> <result file>\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int hdr[7], sp[15];
  double fsc[65];
  rd(f, hdr, 7);
  rd(f, sp, 15);
  rd(f, fsc, 65);
  const int rows = hdr[0], N = hdr[1], frame_first = hdr[2], frame_every = hdr[3], T = hdr[4], has_done = hdr[5], C = hdr[6];
  irrl_eval_spectrum_spec s;
  s.x_dim = sp[0]; s.x_first = sp[1]; s.x_count = sp[2]; s.nperseg = sp[3]; s.hop = sp[4]; s.detrend = sp[5]; s.matrix_count = sp[6];
  for (int m = 0; m < 8; m++) s.matrix_env[m] = sp[7 + m];
  s.fs = fsc[0];
  for (int c = 0; c < 64; c++) s.scale[c] = fsc[1 + c];
  if (const char *bad = irrl_eval_spectrum_spec_error(s)) { fprintf(stderr, "spec: %s\n", bad); return 3; }
  if (rows < 1 || N < 1 || T < 1 || T > IRRL_EVAL_SPECTRUM_MAX_FRAMES || frame_first < 0 || frame_every < 1 ||
      irrl_eval_recurrence_row(frame_first, frame_every, T - 1) >= rows || C < 1 || N % C != 0) {
    fprintf(stderr, "bad header\n"); return 2;
  }
  for (int m = 0; m < s.matrix_count; m++)
    if (s.matrix_env[m] < 0 || s.matrix_env[m] >= N) { fprintf(stderr, "bad matrix_env\n"); return 2; }
  const int P = s.nperseg, K = irrl_eval_spectrum_bins(P), S_max = irrl_eval_spectrum_segments(T, P, s.hop);
  std::vector<double> window((size_t)P), tw(2 * (size_t)P);
  rd(f, window.data(), window.size());
  rd(f, tw.data(), tw.size());
  std::vector<float> x((size_t)rows * (size_t)N * (size_t)s.x_dim);
  rd(f, x.data(), x.size());
  std::vector<uint8_t> done;
  if (has_done) { done.resize((size_t)rows * (size_t)N); rd(f, done.data(), done.size()); }
  fclose(f);

  const size_t cx = (size_t)s.x_count, G = (size_t)C, R = (size_t)(N / C), Ks = (size_t)K, Ss = (size_t)S_max, M = (size_t)s.matrix_count;
  const double density = irrl_eval_spectrum_density(window.data(), P, s.fs, 0.0);
  std::vector<int64_t> segments(G, 0);
  std::vector<double> psd_sum(G * cx * Ks, 0.0), sxx(M * cx * Ss * Ks, 0.0), part(cx * Ks), v((size_t)P);
  for (size_t g = 0; g < G; g++)
    for (size_t r = 0; r < R; r++) {
      const size_t e = g * R + r;
      int te = T;
      if (has_done)
        for (int i = 0; i < T; i++)
          if (done[(size_t)irrl_eval_recurrence_row(frame_first, frame_every, i) * (size_t)N + e] != 0) { te = i; break; }
      const int Se = irrl_eval_spectrum_segments(te, P, s.hop);
      for (auto &p : part) p = 0.0;
      for (int seg = 0; seg < Se; seg++)                          // the robot's segments in ascending order
        for (size_t c = 0; c < cx; c++) {
          for (int n = 0; n < P; n++) {
            const size_t row = (size_t)irrl_eval_recurrence_row(frame_first, frame_every, seg * s.hop + n);
            v[(size_t)n] = irrl_eval_spectrum_sample(x[(row * (size_t)N + e) * (size_t)s.x_dim + (size_t)s.x_first + c], s.scale[c]);
          }
          const double m = s.detrend ? irrl_eval_spectrum_mean(v.data(), 1, P, 0.0) : 0.0;
          for (int n = 0; n < P; n++) v[(size_t)n] = irrl_eval_spectrum_windowed(v[(size_t)n], m, s.detrend, window[(size_t)n]);
          for (int k = 0; k < K; k++) {
            double re = 0.0, si = 0.0;
            int j = 0;
            for (int n = 0; n < P; n++) {                          // the samples in ascending order
              re = irrl_eval_spectrum_add(re, v[(size_t)n], tw[2 * (size_t)j]);
              si = irrl_eval_spectrum_add(si, v[(size_t)n], tw[2 * (size_t)j + 1]);
              j = irrl_eval_spectrum_step(j, k, P);
            }
            const double p = irrl_eval_spectrum_power(re, si, irrl_eval_spectrum_gain(k, P), density);
            part[c * Ks + (size_t)k] = part[c * Ks + (size_t)k] + p;
            for (size_t mi = 0; mi < M; mi++)
              if ((size_t)s.matrix_env[mi] == e) sxx[((mi * cx + c) * Ss + (size_t)seg) * Ks + (size_t)k] = p;
          }
        }
      segments[g] += Se;                                          // the condition's robots in ascending order
      for (size_t q = 0; q < cx * Ks; q++) psd_sum[g * cx * Ks + q] = psd_sum[g * cx * Ks + q] + part[q];
    }

  f = fopen(argv[2], "wb");
  if (!f) { perror(argv[2]); return 2; }
  wr(f, segments.data(), segments.size());
  wr(f, psd_sum.data(), psd_sum.size());
  wr(f, sxx.data(), sxx.size());
  const uint64_t per = (uint64_t)irrl_eval_spectrum_work_per_env(s);
  wr(f, &per, 1);
  fclose(f);
  return 0;
}
